"""Stress launches of the bf16 convolution family (csrc/conv_mfma.hip, narrow_head.hip, bottleneck_frozen.hip, stem_conv.hip)
at the small and ragged shapes, and at the instantiations, that the audited steps of tests/test_conv_audit.py never launch.

The GPU tests drive the Python entry points tests/conv_audit.py wraps (hip_conv.conv_forward with explicit variants,
conv_dgrad_s2, conv_wgrad, conv_wgrad_parts, wgrad_multi, frozen_bottleneck, the narrow head, hip_ops.stem_conv) with the
auditor installed, in two operand regimes:

1. Integer-exact.  Every operand is a small integer stored in bf16 (bias: fp32 integers), ReLU masks / bits are random.
   Every product and - while S, the same computation over absolute values, stays below 2^24 - every partial sum in any
   order is exact in fp32, so a kernel has exactly ONE admissible output: the integer itself for fp32 outputs (each
   weight-gradient split partial, the reduced weight gradient, column sums), its round-to-nearest-even bf16 value for bf16
   outputs, and with a residual rne(relu(rne(conv + bias) + res)).  Compared with torch.equal (Auditor.exact), on every
   variant.  Each test asserts on its REFERENCE, before comparing, that S < 2^24 and that its bf16 outputs hold at least
   100 exact ties which nearest-even rounds down in magnitude and 100 which it rounds up (truncation and round-half-away
   both fail then).  The tie count is asserted per launch where the launch has at least TIE_ELEMS live outputs, and
   always over the launches of a test: a launch of one pixel has 64 outputs and cannot hold 200 ties.  Column sums and
   weight gradients are fp32 outputs: exact integers, no rounding, hence no tie condition.

2. Trained-like, under the auditor's unchanged bound (RHO, GAMMA, ALPHA): x = relu(N(0, 1)) times a per-channel log-normal
   scale, w = N(0, 1) / sqrt(C R S) with three output channels times 64, biases of several units; a same-signed launch
   (S = |r|) wherever an fp32 output exists; and a scale-invariance pair without bias - the launch on (2^40 x, 2^-37 w) must
   be bit-identical to 2^3 times the launch on (x, w).

Every launch's instantiation is asserted by name (the auditor's name carries the tile width conv_launch takes), and the
last test asserts that the union over the module equals DISPATCH, the table of every instantiation the launchers can
dispatch.  Every test prints the auditor's table.

The CPU self-tests (not ``gpu``) feed fp32 restatements through the same exact check: what it accepts (two summation orders)
and what it rejects (truncation, round-half-away, one dropped product in a corner pixel, one rounding where the contract
has two, a split partial left at zero), and they assert the regime's conditions for every named integer case.
"""
import pytest
import torch

import conv_audit as CA

TIE_ELEMS = 8192        # live bf16 outputs from which ONE launch must hold the 100 + 100 ties on its own
_SEEN = set()           # union of the audited instantiations over this module's GPU tests


# ------------------------------------------------------------------------------------------------------------ operands
def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ints(shape, lim, g, dev, lo=None):
    return torch.randint(-lim if lo is None else lo, lim + 1, shape, generator=g, device=dev).to(torch.float32)


def _lims(n_products):
    """operand ranges by reduction length: wide enough that sums pass 256 (where bf16 starts to round integers)"""
    return (16, 8) if n_products <= 256 else (8, 4)


def out_hw(H, W, R, stride, pad, dil):
    return (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (R - 1) - 1) // stride + 1


def fwd_operands(dev, geo, res, mask, regime, seed=0, bias=True):
    """(x, w, bias, residual, mask, mask_bits) of a forward launch; ``res`` None | 'same' | 'up', ``mask`` None | 'bf16' |
    'bits'; ``regime`` 'int' | 'trained' | 'same-signed'"""
    N, C, H, W, K, R, stride, pad, dil = geo
    g = _gen(dev, 7919 * seed + C + 3 * K + 5 * H + 7 * W + R)
    Ho, Wo = out_hw(H, W, R, stride, pad, dil)
    rshape = (N, K, Ho // 2, Wo // 2) if res == 'up' else (N, K, Ho, Wo)
    if regime == 'int':
        xl, wl = _lims(C * R * R)
        x = _ints((N, C, H, W), xl, g, dev)
        w = _ints((K, C, R, R), wl, g, dev)
        b = _ints((K,), 64, g, dev) if bias else None
        r = _ints(rshape, 64, g, dev) if res else None
    else:
        x = torch.randn((N, C, H, W), generator=g, device=dev).clamp_min(0) * \
            torch.exp(torch.randn((1, C, 1, 1), generator=g, device=dev))
        w = torch.randn((K, C, R, R), generator=g, device=dev) / (C * R * R) ** 0.5
        w[[0, K // 2, K - 1]] *= 64.0
        b = torch.randn((K,), generator=g, device=dev) * 3 if bias else None
        r = torch.randn(rshape, generator=g, device=dev) * 2 if res else None
        if regime == 'same-signed':
            w = w.abs()
            b = b.abs() if b is not None else None
            r = r.abs() if r is not None else None
    m = mb = None
    if mask is not None:
        keep = torch.rand((N, Ho, Wo, K), generator=g, device=dev) < 0.6
        if mask == 'bits':
            mb = CA.pack_bits(keep)
        else:
            m = _cl((keep.permute(0, 3, 1, 2).float() * 2 - 1).to(torch.bfloat16))
    bf = lambda t: None if t is None else _cl(t.to(torch.bfloat16))   # noqa: E731
    return bf(x), bf(w), b, bf(r), m, mb


def assert_regime(S, ties, live_elems, what):
    """the integer regime's conditions on a launch's reference"""
    assert float(S.max()) < CA.EXACT_LIMIT, (what, float(S.max()))
    if live_elems >= TIE_ELEMS:
        assert ties[0] >= 100 and ties[1] >= 100, (what, ties, live_elems)


class Tally:
    """ties (down, up) over the bf16 outputs of a test's launches"""

    def __init__(self):
        self.down = self.up = self.elems = 0

    def add(self, ties, elems):
        self.down += ties[0]
        self.up += ties[1]
        self.elems += elems

    def check(self):
        print('bf16 ties over the test: %d down / %d up of %d live outputs' % (self.down, self.up, self.elems))
        assert self.down >= 100 and self.up >= 100, (self.down, self.up, self.elems)


def finish(A, title, tally=None):
    A.print_table(title)
    _SEEN.update(A.kernels)
    if tally is not None:
        tally.check()
    assert not A.failures, A.failures[:10]


# -------------------------------------------------------------------------------------------- forward / stride-1 dgrad
# (id, (N, C, H, W, K, R, stride, pad, dil), variant, residual, mask, bits out, column sums, relu, instantiation)
T, F_ = True, False
FWD_64 = [
    ('M=1', (1, 64, 1, 1, 64, 1, 1, 0, 1), 3, None, None, F_, F_, F_, 'conv_igemm_kernel<64, false, 1, true>'),
    ('M=127, 1xW, K=192', (1, 64, 1, 127, 192, 3, 1, 1, 1), 3, None, None, F_, F_, T, 'conv_igemm_kernel<64, false, 1, false>'),
    ('M=129, Hx1', (1, 128, 129, 1, 64, 3, 1, 1, 1), 1, None, None, F_, T, F_, 'conv_igemm_kernel<64, false, 2, false>'),
    ('M=255, K=384, residual', (1, 64, 15, 17, 384, 1, 1, 0, 1), 3, 'same', None, F_, F_, T, 'conv_igemm_kernel<64, true, 1, true>'),
    ('M=257, bf16 mask', (1, 64, 1, 257, 128, 3, 1, 1, 1), 1, None, 'bf16', F_, T, F_, 'conv_igemm_kernel<64, true, 2, false>'),
    ('3 images of 5x7 in one tile, bits in / out, column sums', (3, 64, 5, 7, 128, 3, 1, 1, 1), 3, None, 'bits', T, T, F_,
     'conv_igemm_kernel<64, true, 1, false>'),
    ('2x2, dil = pad = 2, C=2048', (2, 2048, 2, 2, 64, 3, 1, 2, 2), 1, None, None, F_, F_, F_, 'conv_igemm_kernel<64, false, 2, false>'),
    ('stride 2, odd', (1, 64, 17, 23, 128, 3, 2, 1, 1), 3, 'same', None, T, F_, T, 'conv_igemm_kernel<64, true, 1, false>'),
    ('stride 2, even', (2, 128, 16, 22, 192, 3, 2, 1, 1), 1, None, None, F_, F_, T, 'conv_igemm_kernel<64, false, 2, false>'),
    ('3x3, C=64, K=128, 17x23', (1, 64, 17, 23, 128, 3, 1, 1, 1), 0, None, None, F_, F_, F_, 'conv_igemm_kernel<64, false, 1, false>'),
    ('3x3 dilated, C=2048, K=512, 12x12', (1, 2048, 12, 12, 512, 3, 1, 2, 2), 0, None, None, F_, F_, T,
     'conv_igemm_kernel<64, false, 2, false>'),
    ('1x1, C=64, K=256, 9x11', (1, 64, 9, 11, 256, 1, 1, 0, 1), 0, None, None, F_, F_, F_, 'conv_igemm_kernel<64, false, 1, true>'),
    ('1x1, bits in, column sums on a partial tile', (1, 128, 9, 15, 64, 1, 1, 0, 1), 3, None, 'bits', F_, T, F_,
     'conv_igemm_kernel<64, true, 1, true>'),
]
# the 128-wide tile: ceil(M / 128) (K / 128) > 256 - 97 x 89 = 8633 pixels (68 tiles, the last one of 57 pixels) x K = 512
G128 = (1, 64, 97, 89, 512)
FWD_128 = [
    ('3x3', G128 + (3, 1, 1, 1), 3, None, None, F_, F_, T, 'conv_igemm_kernel<128, false, 1, false>'),
    ('3x3, residual, bits out', G128 + (3, 1, 1, 1), 3, 'same', None, T, F_, T, 'conv_igemm_kernel<128, true, 1, false>'),
    ('3x3, two stages, column sums', G128 + (3, 1, 1, 1), 1, None, None, F_, T, F_, 'conv_igemm_kernel<128, false, 2, false>'),
    ('3x3, two stages, bits in', G128 + (3, 1, 1, 1), 1, None, 'bits', F_, T, F_, 'conv_igemm_kernel<128, true, 2, false>'),
    ('1x1', G128 + (1, 1, 0, 1), 3, None, None, T, F_, T, 'conv_igemm_kernel<128, false, 1, true>'),
    ('1x1, bits in / out, column sums', G128 + (1, 1, 0, 1), 3, None, 'bits', T, T, F_,
     'conv_igemm_kernel<128, true, 1, true>'),
]
FWD_256 = [
    ('K=256, ragged', (1, 64, 17, 23, 256, 3, 1, 1, 1), 2, None, None, F_, T, T, 'conv_igemm256_kernel<false, 2>'),
    ('K=512, M=257, residual', (1, 128, 1, 257, 512, 1, 1, 0, 1), 2, 'same', None, T, F_, T, 'conv_igemm256_kernel<true, 2>'),
    ('K=128: 256 x 128 tile', (3, 64, 5, 7, 128, 3, 1, 1, 1), 2, None, None, F_, F_, F_, 'conv_igemm256_kernel<false, 1>'),
    ('K=384, stride 2, bits in, column sums', (1, 128, 33, 31, 384, 3, 2, 1, 1), 2, None, 'bits', F_, T, F_,
     'conv_igemm256_kernel<true, 1>'),
    ('K=384, 1x1, M=255, bf16 mask', (1, 64, 15, 17, 384, 1, 1, 0, 1), 2, None, 'bf16', F_, F_, F_, 'conv_igemm256_kernel<true, 1>'),
]
# the streaming kernel: (C, K, sp); M0 = 16384 is the smallest pixel count it takes at these K (csrc pw_stream_ranges:
# M % sp == 0 and M / sp >= 8 * 512 / ncol), M0 + sp leaves its pixel ranges uneven
STREAM = {64: (2048, 32), 128: (2048, 32), 256: (1024, 16), 512: (512, 16)}
STREAM_HW = {16384: (128, 128), 16416: (96, 171), 16400: (100, 164)}
STREAM_FORMS = [(None, None, F_), ('same', None, F_), ('same', 'bits', F_), ('same', None, T), (None, 'bits', F_), (None, None, T)]


def stream_cases(C):
    K, sp = STREAM[C]
    out = []
    for M in (16384, 16384 + sp):
        H, W = STREAM_HW[M]
        for res, mask, bout in STREAM_FORMS:
            name = 'conv_pw_stream_kernel<%d, %s, %s, %s>' % (C, 'true' if res else 'false', 'true' if mask else 'false',
                                                              'true' if bout else 'false')
            out.append(('M=%d' % M, (1, C, H, W, K, 1, 1, 0, 1), 4 if res else 0, res, mask, bout, not bout, res is not None, name))
    if C == 256:      # the FPN top-down add in the epilogue: power-of-two map (shifts) and not (divisions)
        for M in (16384, 16400):
            H, W = STREAM_HW[M]
            out.append(('M=%d, res_up' % M, (1, C, H, W, K, 1, 1, 0, 1), 0, 'up', None, F_, F_, F_,
                        'conv_pw_stream_kernel<256, true, false, false>'))
    return out


def forward_launch(A, hc, case, regime, tally=None, seed=0, bias=True, ops=None):
    """one audited conv_forward launch; integer regime: + the exact comparisons.  Returns (y, column sums, operands)."""
    cid, geo, variant, res, mask, bout, colsum, relu, name = case
    N, C, H, W, K, R, stride, pad, dil = geo
    dev = A.dev
    A.regime = regime
    x, w, b, r, m, mb = ops if ops is not None else fwd_operands(dev, geo, res, mask, regime, seed, bias)
    Ho, Wo = out_hw(H, W, R, stride, pad, dil)
    bo = torch.full((N * Ho * Wo * K // 8,), 0xa5, dtype=torch.uint8, device=dev) if bout else None
    if regime == 'int':
        yr, S, first, live = CA.forward_exact(x, w, b, r, stride, pad, dil, relu, m, mb, res == 'up')
        ties, n_live = CA.bf16_ties(first, live), int(live.sum())
        assert_regime(S, ties, n_live, (cid, name))
        if tally is not None:
            tally.add(ties, n_live)
    out = hc.conv_forward(x, w, b, r, stride, pad, dil, relu, variant=variant, mask=m, want_colsum=colsum, mask_bits=mb,
                          bits_out=bo, res_up=res == 'up')
    torch.cuda.synchronize()
    assert A.last == name, (cid, A.last, name)
    y, cs = out if colsum else (out, None)
    if regime == 'int':
        shape = tuple(x.shape) + tuple(w.shape)
        A.exact(name, shape, CA._nhwc64(y), yr)
        if bout:
            A.exact(name, shape, bo, CA.pack_bits(yr > 0), check='exact integers: bits_out')
        if colsum:
            flat = yr.reshape(-1, K)
            assert float(flat.abs().sum(0).max()) < CA.EXACT_LIMIT
            A.exact(name, shape, cs, flat.sum(0), check='exact integers: colsum (+reduce)')
    return y, cs, (x, w, b, r, m, mb)


def scale_pair(A, hc, case, seed=1):
    """no bias: the launch on (2^40 x, 2^-37 w) is bit-identical to 2^3 x the launch on (x, w) - powers of two commute with
    every rounding while all values stay normal.  (A residual does not scale with the product: forms with one are skipped.)"""
    cid, geo, variant, res, mask, bout, colsum, relu, name = case
    if res:
        return
    y1, _, (x, w, b, r, m, mb) = forward_launch(A, hc, case, 'trained', seed=seed, bias=False)
    x2 = _cl((x.float() * 2.0 ** 40).to(torch.bfloat16))
    w2 = _cl((w.float() * 2.0 ** -37).to(torch.bfloat16))
    assert torch.equal(x2.float() * 2.0 ** -40, x.float()) and torch.equal(w2.float() * 2.0 ** 37, w.float())
    y2, _, _ = forward_launch(A, hc, case, 'trained', bias=False, ops=(x2, w2, None, None, m, mb))
    assert A.exact(name, tuple(x.shape) + tuple(w.shape), y2.float(), y1.float() * 8.0, check='scale pair 2^40, 2^-37')


def _auditor(dev, monkeypatch):
    from oadg_amd import hip_conv
    A = CA.Auditor().install(monkeypatch)
    A.dev = dev
    return A, hip_conv


def _run_forward_family(dev, monkeypatch, cases, title, trained=lambda i: True):
    A, hc = _auditor(dev, monkeypatch)
    tally = Tally()
    for i, case in enumerate(cases):
        forward_launch(A, hc, case, 'int', tally)
        if trained(i):
            forward_launch(A, hc, case, 'trained')
            if case[6]:                      # an fp32 output (column sums): the same-signed launch
                forward_launch(A, hc, case, 'same-signed', seed=2)
            scale_pair(A, hc, case)
    finish(A, title, tally)
    want = {c[-1] for c in cases}
    assert want <= A.kernels, want - A.kernels


@pytest.mark.gpu
def test_forward_64_wide_tile_at_ragged_shapes(dev, monkeypatch):
    """conv_igemm_kernel<64, ...>: every small shape takes it (conv_launch: ceil(M / 128) K / 128 <= 256).  M = 1, 127, 129,
    255, 257; 1 x W and H x 1 maps; three 5 x 7 images inside one pixel tile under a 3 x 3 filter (halo rows must not cross
    images); a 2 x 2 map with dil = pad = 2 (only the centre tap in bounds); stride 2 on odd and even sizes; C = 64 and 2048;
    K = 64, 192, 384; mask bits in, bits out and column sums on a partial tile; the three shapes of the issue's table."""
    _run_forward_family(dev, monkeypatch, FWD_64, '64-wide tile')


@pytest.mark.gpu
def test_forward_128_wide_tile_every_form(dev, monkeypatch):
    """conv_igemm_kernel<128, post, 1 | 2, pw> in its six forms at the smallest map that takes the 128-wide tile with
    K = 512: 97 x 89 (68 pixel tiles x 4 > 256; the last tile holds 57 pixels)"""
    _run_forward_family(dev, monkeypatch, FWD_128, '128-wide tile')


@pytest.mark.gpu
def test_forward_256_tile_both_widths(dev, monkeypatch):
    """conv_igemm256_kernel<post, 2> and <post, 1> (explicit variant 2 with K % 256 != 0: K = 128 and 384) at M = 105, 255,
    257, 391 and a stride-2 map"""
    _run_forward_family(dev, monkeypatch, FWD_256, '256-pixel tile')


@pytest.mark.gpu
@pytest.mark.parametrize('C', sorted(STREAM))
def test_forward_streaming_kernel_six_operand_forms(dev, monkeypatch, C):
    """conv_pw_stream_kernel<C, res, bits in, bits out> in the six forms launch_pw_stream dispatches, at the smallest pixel
    count the kernel takes and at that + sp (uneven ranges); C = 256 also with the res_up epilogue on a power-of-two map
    and on 100 x 164.  Integer regime on every case; the trained-like launches on the six forms at the uneven pixel count
    and on the res_up pair."""
    cases = stream_cases(C)
    _run_forward_family(dev, monkeypatch, cases, 'streaming kernel, C = %d' % C, trained=lambda i: i >= 6)


# ------------------------------------------------------------------------------------------------ stride-2 data gradient
# (id, N, C, H, W, K, R, accumulate, mask, column sums, instantiation)
S2_CASES = [
    ('3x3, even: four equal classes interleaved', 2, 64, 8, 10, 64, 3, F_, None, F_, 'conv_igemm_s2_kernel<64, false>'),
    ('3x3, odd: unequal classes, C=192, bits, column sums', 2, 192, 9, 11, 128, 3, F_, 'bits', T, 'conv_igemm_s2_kernel<64, true>'),
    ('3x3, H=1: classes skipped, bf16 mask', 4, 128, 1, 9, 64, 3, F_, 'bf16', T, 'conv_igemm_s2_kernel<128, true>'),
    ('3x3, W=1: classes skipped', 4, 128, 7, 1, 64, 3, F_, None, F_, 'conv_igemm_s2_kernel<128, false>'),
    ('3x3, even, C=128, column sums', 1, 128, 12, 16, 128, 3, F_, None, T, 'conv_igemm_s2_kernel<128, false>'),
    ('1x1, accumulate aliasing dx', 2, 128, 9, 7, 256, 1, T, None, F_, 'conv_igemm_s2_kernel<128, true>'),
    ('1x1, bits, column sums', 2, 64, 8, 8, 64, 1, F_, 'bits', T, 'conv_igemm_s2_kernel<64, true>'),
    ('1x1, C=192, odd', 2, 192, 7, 5, 64, 1, F_, None, F_, 'conv_igemm_s2_kernel<64, false>'),
]


def s2_operands(dev, case, regime, seed=0):
    cid, N, C, H, W, K, R, acc, mask, colsum, name = case
    g = _gen(dev, 104729 * seed + C + 3 * K + 5 * H + 7 * W + R)
    pad = 1 if R == 3 else 0
    Ho, Wo = out_hw(H, W, R, 2, pad, 1)
    if regime == 'int':
        gl, wl = _lims(K * R * R // (1 if R == 1 else 2))
        gy, w = _ints((N, K, Ho, Wo), gl, g, dev), _ints((K, C, R, R), wl, g, dev)
        a = _ints((N, C, H, W), 64, g, dev) if acc else None
    else:
        gy = torch.randn((N, K, Ho, Wo), generator=g, device=dev) * torch.exp(torch.randn((1, K, 1, 1), generator=g, device=dev))
        w = torch.randn((K, C, R, R), generator=g, device=dev) / (K * R * R) ** 0.5
        w[:, [0, C // 2, C - 1]] *= 64.0
        a = torch.randn((N, C, H, W), generator=g, device=dev) * 2 if acc else None
        if regime == 'same-signed':
            gy, w = gy.abs(), w.abs()
    m = mb = None
    if mask is not None:
        keep = torch.rand((N, H, W, C), generator=g, device=dev) < 0.6
        if mask == 'bits':
            mb = CA.pack_bits(keep)
        else:
            m = _cl((keep.permute(0, 3, 1, 2).float() * 2 - 1).to(torch.bfloat16))
    return _cl(gy.to(torch.bfloat16)), w, (None if a is None else _cl(a.to(torch.bfloat16))), m, mb


def s2_launch(A, hc, case, regime, tally=None, seed=0, ops=None):
    cid, N, C, H, W, K, R, acc, mask, colsum, name = case
    gy, w, a, m, mb = ops if ops is not None else s2_operands(A.dev, case, regime, seed)
    A.regime = regime
    wf, _, wt = hc.prepared(w, None, None, 2)              # (the class filters; wf = the bf16 forward filters)
    pad = 1 if R == 3 else 0
    acc0 = a.clone() if a is not None else None
    if regime == 'int':
        assert torch.equal(wf.float(), w)
        yr, S, first, live = CA.dgrad_s2_exact(gy, wf, H, W, pad, acc0, m, mb)
        ties, n_live = CA.bf16_ties(first, live), int(live.sum())
        assert_regime(S, ties, n_live, (cid, name))
        tally.add(ties, n_live)
    out = hc.conv_dgrad_s2(gy, wt, (N, C, H, W), R, mask=m, want_colsum=colsum, mask_bits=mb, accumulate=a)
    torch.cuda.synchronize()
    assert A.last == name, (cid, A.last, name)
    gx, cs = out if colsum else (out, None)
    if acc:
        assert gx.data_ptr() == a.data_ptr()
    if regime == 'int':
        shape = tuple(gy.shape) + (C, R)
        A.exact(name, shape, CA._nhwc64(gx), yr)
        if colsum:
            flat = yr.reshape(-1, C)
            assert float(flat.abs().sum(0).max()) < CA.EXACT_LIMIT
            A.exact(name, shape, cs, flat.sum(0), check='exact integers: colsum (+reduce)')
    return gx, (gy, w, acc0, m, mb)


@pytest.mark.gpu
def test_stride2_data_gradient_every_class_layout(dev, monkeypatch):
    """conv_igemm_s2_kernel<64 | 128, post>: R = 3 and 1; C = 64, 192 (64-wide) and 128; even sizes (four equal classes: the
    interleaved path), odd sizes (unequal classes), H = 1 and W = 1 (classes skipped); ``accumulate`` aliasing dx, bf16 mask,
    mask bits and column sums"""
    A, hc = _auditor(dev, monkeypatch)
    tally = Tally()
    for case in S2_CASES:
        s2_launch(A, hc, case, 'int', tally)
        s2_launch(A, hc, case, 'trained')
        if case[9]:
            s2_launch(A, hc, case, 'same-signed', seed=2)
        if not case[7]:      # scale pair (no deposit: it would not scale)
            g1, (gy, w, _, m, mb) = s2_launch(A, hc, case, 'trained', seed=3)
            gy2 = _cl((gy.float() * 2.0 ** 40).to(torch.bfloat16))
            w2 = w.to(torch.bfloat16).float() * 2.0 ** -37
            g2, _ = s2_launch(A, hc, case, 'trained', ops=(gy2, w2, None, m, mb))
            assert A.exact(case[-1], gy.shape, g2.float(), g1.float() * 8.0, check='scale pair 2^40, 2^-37')
    finish(A, 'stride-2 data gradient', tally)
    assert {c[-1] for c in S2_CASES} <= A.kernels


# ------------------------------------------------------------------------------------------------------ weight gradient
# (id, N, C, H, W, K, R, stride, pad, dil, kernel, splits that own no pixel)
WG_CASES = [
    ('1x1, P=50 < one chunk', 2, 128, 5, 5, 128, 1, 1, 0, 1, 'conv_wgrad_kernel<2>', 0),
    ('1x1, P=63', 1, 128, 1, 63, 128, 1, 1, 0, 1, 'conv_wgrad_kernel<2>', 0),
    ('1x1, P=64', 1, 128, 8, 8, 256, 1, 1, 0, 1, 'conv_wgrad_kernel<2>', 0),
    ('1x1, P=65', 1, 256, 5, 13, 128, 1, 1, 0, 1, 'conv_wgrad_kernel<2>', 0),
    ('1x1, 33 chunks over 8 splits of 5: one split empty', 1, 128, 49, 43, 128, 1, 1, 0, 1, 'conv_wgrad_kernel<2>', 1),
    ('3x3, 33 chunks over 8 splits of 5', 1, 128, 49, 43, 128, 3, 1, 1, 1, 'conv_wgrad_kernel<1>', 1),
    ('3x3, stride 2', 1, 128, 33, 31, 128, 3, 2, 1, 1, 'conv_wgrad_kernel<1>', 0),
    ('3x3, dilation 2', 1, 128, 20, 21, 256, 3, 1, 2, 2, 'conv_wgrad_kernel<1>', 0),
    ('256-tile, row strips crossing images', 3, 256, 75, 64, 256, 3, 1, 1, 1, 'conv_wgrad256_kernel', 0),
    ('256-tile, 227 chunks over 28 splits of 9: two splits empty', 1, 256, 120, 121, 256, 3, 1, 1, 1, 'conv_wgrad256_kernel', 2),
    ('256-tile, stride 2, row strips', 2, 256, 226, 128, 256, 3, 2, 1, 1, 'conv_wgrad256_kernel', 0),
    ('256-tile, dilation 2', 1, 256, 120, 121, 256, 3, 1, 2, 2, 'conv_wgrad256_kernel', 2),
    ('256-tile, 1x1, 1024 chunks over 128 splits, the last chunk ragged', 1, 256, 255, 257, 512, 1, 1, 0, 1, 'conv_wgrad256_kernel', 0),
]


def wg_operands(dev, geo, regime, seed=0):
    N, C, H, W, K, R, stride, pad, dil = geo
    g = _gen(dev, 1299709 * seed + C + 3 * K + 5 * H + 7 * W + R + stride + dil)
    Ho, Wo = out_hw(H, W, R, stride, pad, dil)
    if regime == 'int':
        x, gy = _ints((N, C, H, W), 8, g, dev), _ints((N, K, Ho, Wo), 8, g, dev)
    else:
        x = torch.randn((N, C, H, W), generator=g, device=dev).clamp_min(0) * \
            torch.exp(torch.randn((1, C, 1, 1), generator=g, device=dev))
        gy = torch.randn((N, K, Ho, Wo), generator=g, device=dev) * 1e-3
        gy[:, [0, K // 2, K - 1]] *= 64.0
        if regime == 'same-signed':
            gy = gy.abs()
    return _cl(x.to(torch.bfloat16)), _cl(gy.to(torch.bfloat16))


def _parts_view(ws, off, splits, K, RS, C):
    return ws[off:off + splits * K * RS * C * 4].view(torch.float32).view(splits, K, RS, C)


def check_parts_exact(A, name, x, gy, geo, parts, pix, empty=None):
    """EACH split partial against the gradient over its own pixel range (a partial that owns no pixel: zeros)"""
    N, C, H, W, K, R, stride, pad, dil = geo
    splits = parts.shape[0]
    ref, S = CA.wgrad_parts_exact(x, gy, R, R, stride, pad, dil, splits, pix)
    assert float(S.max()) < CA.EXACT_LIMIT
    P = gy.shape[0] * gy.shape[2] * gy.shape[3]
    n_empty = sum(1 for s in range(splits) if s * pix >= P)
    if empty is not None:
        assert n_empty == empty, (n_empty, empty, splits, pix, P)
    shape = tuple(x.shape) + (K, R, stride, dil)
    for s in range(splits):
        A.exact(name, shape, parts[s], ref[s], check='exact integers: split partial')
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize('case', WG_CASES, ids=[c[0] for c in WG_CASES])
def test_weight_gradient_every_split_partial(dev, monkeypatch, case):
    """conv_wgrad_kernel<2> (1x1), <1> (3x3) and conv_wgrad256_kernel: P below one 64-pixel chunk, one chunk +- 1, chunk
    counts that are no multiple of the split count (the partial of a split that owns no chunk must be zeros: every partial is
    compared, not their sum), the row-strip form with rows crossing image boundaries inside a split, stride 2, dilation 2;
    conv_wgrad's reduced result on the same operands"""
    cid, N, C, H, W, K, R, stride, pad, dil, kernel, empty = case
    geo = (N, C, H, W, K, R, stride, pad, dil)
    A, hc = _auditor(dev, monkeypatch)
    L = hc._lib.lib()
    Ho, Wo = out_hw(H, W, R, stride, pad, dil)
    x, gy = wg_operands(dev, geo, 'int')
    A.regime = 'int'
    ws, splits = hc.conv_wgrad_parts(x, gy, K, R, R, stride, pad, dil)
    torch.cuda.synchronize()
    assert A.last == kernel, (A.last, kernel)
    pix = CA.wgrad_split_geometry(L, N, Ho, Wo, C, K, R, R, splits)
    ref = check_parts_exact(A, kernel, x, gy, geo, _parts_view(ws, 0, splits, K, R * R, C), pix, empty)
    dw = hc.conv_wgrad(x, gy, K, R, R, stride, pad, dil)
    torch.cuda.synchronize()
    assert A.last == kernel + ' (+reduce)'
    A.exact(kernel + ' (+reduce)', tuple(x.shape) + (K, R, stride, dil), dw.permute(0, 2, 3, 1).reshape(K, R * R, C), ref.sum(0))
    for regime in ('trained', 'same-signed'):
        xt, gt = wg_operands(dev, geo, regime, seed=1)
        A.regime = regime
        ws1, sp1 = hc.conv_wgrad_parts(xt, gt, K, R, R, stride, pad, dil)
        hc.conv_wgrad(xt, gt, K, R, R, stride, pad, dil)
    # scale pair on the last (same-signed) operands: every partial bit-identical to 2^3 x
    x2 = _cl((xt.float() * 2.0 ** 40).to(torch.bfloat16))
    g2 = _cl((gt.float() * 2.0 ** -37).to(torch.bfloat16))
    assert torch.equal(g2.float() * 2.0 ** 37, gt.float())
    ws2, sp2 = hc.conv_wgrad_parts(x2, g2, K, R, R, stride, pad, dil)
    torch.cuda.synchronize()
    assert sp1 == sp2 == splits
    p1, p2 = _parts_view(ws1, 0, splits, K, R * R, C), _parts_view(ws2, 0, splits, K, R * R, C)
    assert A.exact(kernel, tuple(x.shape) + (K, R, stride, dil), p2, p1 * 8.0, check='scale pair 2^40, 2^-37')
    finish(A, 'weight gradient, %s' % cid)


def multi_plan(hc, jobs, target):
    """[(splits, pixels per split)] of a grouped launch: the host plan wgrad_multi itself calls, on the same job table"""
    import ctypes
    import numpy as np
    tab = np.zeros(len(jobs), dtype=hc._lib.WGRAD_JOB)
    for r, (x16, gy16, K, R, S_, stride, pad, dil) in zip(tab, jobs):
        N, C, H, W = x16.shape
        r['N'], r['H'], r['W'], r['C'], r['K'], r['R'], r['S'] = N, H, W, C, K, R, S_
        r['stride'], r['pad'], r['dil'] = stride, pad, dil
    first = (ctypes.c_int * 9)()
    assert hc._lib.lib().oadg_conv2d_wgrad_multi_plan(tab.ctypes.data_as(ctypes.c_void_p), len(jobs), int(target), first) > 0
    return [(int(r['splits']), int(r['chunks_per_split']) * 64) for r in tab]


MULTI_GEO = [(1, 256, 5, 10, 256, 1, 1, 0, 1),          # one chunk (50 pixels)
             (2, 256, 40, 37, 512, 3, 1, 1, 1),         # 2960 pixels, 47 chunks, 18 weight tiles
             (1, 512, 9, 64, 256, 3, 1, 1, 1)]          # row strips (Wo = 64)


@pytest.mark.gpu
@pytest.mark.parametrize('target', [256, 7])
def test_grouped_weight_gradient_every_split_partial(dev, monkeypatch, target):
    """conv_wgrad256_multi_kernel: a one-chunk job beside a large one and a row-strip one, planned for 256 workgroups and for
    7 (more weight tiles than workgroups: one split each); every split partial of every job"""
    A, hc = _auditor(dev, monkeypatch)
    for regime in ('int', 'trained', 'same-signed'):
        ops = [wg_operands(dev, geo, regime, seed=3) for geo in MULTI_GEO]
        A.regime = regime
        jobs = [(x, gy) + geo[4:6] + geo[5:] for (x, gy), geo in zip(ops, MULTI_GEO)]
        plan = multi_plan(hc, jobs, target)
        ws, parts = hc.wgrad_multi(jobs, target)
        torch.cuda.synchronize()
        assert A.last == 'conv_wgrad256_multi_kernel'
        if regime != 'int':
            continue
        for (x, gy), geo, (p, splits), (sp, pix) in zip(ops, MULTI_GEO, parts, plan):
            assert splits == sp
            N, C, H, W, K, R = geo[:6]
            check_parts_exact(A, 'conv_wgrad256_multi_kernel', x, gy, geo,
                              _parts_view(ws, p - ws.data_ptr(), splits, K, R * R, C), pix)
    finish(A, 'grouped weight gradient, target %d' % target)


# ------------------------------------------------------------------------------------- narrow head, frozen block, stem
NARROW_M = (1, 63, 65, 4 * 13 * 7 + 3)


@pytest.mark.gpu
@pytest.mark.parametrize('C', [128, 256])
def test_narrow_head_forward_and_backward(dev, monkeypatch, C):
    """n16_fwd / n16_dgrad / n16_wgrad_kernel<C> through hip_conv.narrow_head (15 live output channels) at M = 1, 63, 65 and
    4 * 13 * 7 + 3.  (M = 1 has 16 outputs: the tie count is asserted over the test.)"""
    A, hc = _auditor(dev, monkeypatch)
    tally = Tally()
    for M in NARROW_M:
        for regime in ('int', 'trained', 'same-signed'):
            g = _gen(dev, 31 * M + C + len(regime))
            A.regime = regime
            if regime == 'int':
                x, w = _ints((1, C, 1, M), 16, g, dev), _ints((15, C, 1, 1), 8, g, dev)
                b, gy = _ints((15,), 64, g, dev), _ints((1, 16, 1, M), 64, g, dev)
            else:
                x = torch.randn((1, C, 1, M), generator=g, device=dev).clamp_min(0) * \
                    torch.exp(torch.randn((1, C, 1, 1), generator=g, device=dev))
                w = torch.randn((15, C, 1, 1), generator=g, device=dev) / C ** 0.5
                w[[0, 7, 14]] *= 64.0
                b = torch.randn((15,), generator=g, device=dev) * 3
                gy = torch.randn((1, 16, 1, M), generator=g, device=dev) * 1e-2
                if regime == 'same-signed':
                    w, gy = w.abs(), gy.abs()
            gy[:, 15] = 0
            w = w.to(torch.bfloat16).float().requires_grad_(True)
            b = b.requires_grad_(True)
            x = _cl(x.to(torch.bfloat16)).requires_grad_(True)
            gy = _cl(gy.to(torch.bfloat16))
            w16, wt16, b16 = hc.narrow_params(w, b)
            y = hc.narrow_head(x, w, b, w16, wt16, b16)
            y.backward(gy)
            torch.cuda.synchronize()
            if regime != 'int':
                continue
            x64, g64 = CA._nhwc64(x).reshape(M, C), CA._nhwc64(gy).reshape(M, 16)
            w64, b64 = w16.double(), b16.double()
            first = x64 @ w64.t() + b64
            S = x64.abs() @ w64.abs().t() + b64.abs()
            live = torch.ones_like(first, dtype=torch.bool)
            live[:, 15] = False
            tally.add(CA.bf16_ties(first, live), 15 * M)
            gfirst = g64 @ w64
            tally.add(CA.bf16_ties(gfirst), M * C)
            Sw = g64.abs().t() @ x64.abs()
            assert max(float(S.max()), float((g64.abs() @ w64.abs()).max()), float(Sw.max())) < CA.EXACT_LIMIT
            shape = (M, C)
            A.exact('n16_fwd_kernel<%d>' % C, shape, CA._nhwc64(y).reshape(M, 16), CA.bf16_rne(first))
            A.exact('n16_dgrad_kernel<%d>' % C, shape, CA._nhwc64(x.grad).reshape(M, C), CA.bf16_rne(gfirst))
            A.exact('n16_wgrad_kernel<%d>' % C, shape, w.grad.reshape(15, C), (g64.t() @ x64)[:15])
            A.exact('n16_wgrad_kernel<%d>' % C, shape, b.grad, g64.sum(0)[:15], check='exact integers: bias')
    finish(A, 'narrow head, C = %d' % C, tally)
    assert {'n16_%s_kernel<%d>' % (k, C) for k in ('fwd', 'dgrad', 'wgrad')} <= A.kernels


def frozen_block(dev, first, regime, seed=0):
    from oadg_amd.backbones import Bottleneck, make_res_layer
    g = _gen(dev, 17 + seed + int(first))
    if first:
        blk = make_res_layer(64, 64, 1, 1, 1, 'pytorch', dict(type='BN'))[0].to(dev).eval()
    else:
        blk = Bottleneck(256, 64).to(dev).eval()
    convs = [blk.conv1, blk.conv2, blk.conv3] + ([blk.downsample[0]] if first else [])
    bns = [blk.bn1, blk.bn2, blk.bn3] + ([blk.downsample[1]] if first else [])
    with torch.no_grad():
        for conv, bn, density in zip(convs, bns, (1.0, 0.25, 0.5, 1.0)):
            shape = conv.weight.shape
            if regime == 'int':
                # ternary, conv2 / conv3 sparse: S stays below 2^24 through the three stages; a fold that is the identity
                # (gamma = 1, mean = 0, var = 1, eps = 0) keeps the weights and the bias integers
                wv = _ints(shape, 1, g, dev) * (torch.rand(shape, generator=g, device=dev) < density)
                conv.weight.copy_(wv)
                bn.eps = 0.0
                bn.weight.fill_(1.0)
                bn.running_mean.zero_()
                bn.running_var.fill_(1.0)
                bn.bias.copy_(_ints((shape[0],), 16, g, dev))
            else:
                conv.weight.copy_(torch.randn(shape, generator=g, device=dev) / (shape[1] * shape[2] * shape[3]) ** 0.5)
                bn.weight.copy_(torch.rand(shape[0], generator=g, device=dev) + 0.5)
                bn.weight[[0, shape[0] // 2]] *= 8.0
                bn.bias.copy_(torch.randn(shape[0], generator=g, device=dev))
                bn.running_mean.copy_(torch.randn(shape[0], generator=g, device=dev) * 0.2)
                bn.running_var.copy_(torch.rand(shape[0], generator=g, device=dev) + 0.5)
    for p in blk.parameters():
        p.requires_grad_(False)
    return blk, convs, bns


FROZEN_SHAPES = ((1, 1, 1), (1, 5, 7), (3, 9, 9))


@pytest.mark.gpu
@pytest.mark.parametrize('first', [False, True])
def test_frozen_block_both_kinds(dev, monkeypatch, first):
    """bottleneck_frozen_kernel (identity) / bottleneck_frozen_first_kernel (1x1 convolution on the shortcut) at (1, 1, 1),
    (1, 5, 7) and (3, 9, 9): t1, t2 and the shortcut rounded as frozen_block_expect documents"""
    A, hc = _auditor(dev, monkeypatch)
    name = 'bottleneck_frozen_first_kernel' if first else 'bottleneck_frozen_kernel'
    cin = 64 if first else 256
    tally = Tally()
    hc.enable(True)
    try:
        for regime in ('int', 'trained'):
            blk, convs, bns = frozen_block(dev, first, regime)
            A.regime = regime
            for N, H, W in FROZEN_SHAPES:
                g = _gen(dev, N + H + W)
                if regime == 'int':
                    x = _ints((N, cin, H, W), 8, g, dev)
                else:
                    x = torch.randn((N, cin, H, W), generator=g, device=dev).clamp_min(0) * \
                        torch.exp(torch.randn((1, cin, 1, 1), generator=g, device=dev))
                x = _cl(x.to(torch.bfloat16))
                y = hc.frozen_bottleneck(x, blk)
                assert y is not None
                torch.cuda.synchronize()
                assert A.last == name
                if regime != 'int':
                    continue
                prep = [hc.prepared(c.weight, bn, None, 0, c) for c, bn in zip(convs, bns)]
                for (wf, b, _), c, bn in zip(prep, convs, bns):          # the fold left integers
                    assert torch.equal(wf.float(), c.weight) and torch.equal(b, bn.bias)
                yr, Ss, firsts, live = CA.frozen_block_exact(x, [p[0] for p in prep], [p[1] for p in prep], first)
                assert max(float(S.max()) for S in Ss) < CA.EXACT_LIMIT
                # the ties of the LAST rounding's input: bf16(conv3 + b3) + shortcut, where the output is live
                t3 = CA.bf16_rne(firsts[2]) + (CA._nhwc64(x) if not first else
                                              CA.bf16_rne(CA.conv_ref(x, prep[3][0], 1, 0, 1)[0] + prep[3][1].double()))
                ties = CA.bf16_ties(t3, live)
                if int(live.sum()) >= TIE_ELEMS:
                    assert ties[0] >= 100 and ties[1] >= 100, ties
                tally.add(ties, int(live.sum()))
                A.exact(name, x.shape, CA._nhwc64(y), yr)
    finally:
        hc.enable(False)
    finish(A, name, tally)


@pytest.mark.gpu
def test_stem_at_5x6_and_9x130(dev, monkeypatch):
    """stem_conv7x7s2_kernel (147 products per output)"""
    from oadg_amd import hip_ops
    A, hc = _auditor(dev, monkeypatch)
    tally = Tally()
    for N, H, W in ((2, 5, 6), (1, 9, 130)):
        for regime in ('int', 'trained'):
            g = _gen(dev, H + W + len(regime))
            A.regime = regime
            if regime == 'int':
                x, w = _ints((N, 3, H, W), 16, g, dev), _ints((64, 3, 7, 7), 8, g, dev)
            else:
                x = torch.randn((N, 3, H, W), generator=g, device=dev) * 2
                w = torch.randn((64, 3, 7, 7), generator=g, device=dev) / 12
                w[[0, 32, 63]] *= 64.0
            x = _cl(x.to(torch.bfloat16))
            y = hip_ops.stem_conv(x, hip_ops.stem_weights(w))
            torch.cuda.synchronize()
            if regime == 'int':
                yr, S, first, live = CA.forward_exact(x, w.to(torch.bfloat16), None, None, 2, 3, 1, False)
                ties = CA.bf16_ties(first, live)
                assert_regime(S, ties, int(live.sum()), 'stem')
                tally.add(ties, int(live.sum()))
                A.exact('stem_conv7x7s2_kernel', x.shape, CA._nhwc64(y), yr)
    finish(A, 'stem', tally)
    assert 'stem_conv7x7s2_kernel' in A.kernels


# ------------------------------------------------------------------------------------------------------- dispatch table
# Every instantiation the launchers of conv_mfma.hip (convolutions, weight gradients) and narrow_head.hip can dispatch,
# plus the frozen block and the stem.  conv_launch: tile family `conv_igemm_kernel<TB, PO, NS>` / `<TB, PO, 1, true>` (the
# pointwise form exists for one stage only: `pw = one && ...`), `conv_igemm256_kernel<PO, NW_>`, launch_pw_stream's six
# OADG_PWS forms per C (it returns EARG for mask bits in AND bits out: no instantiation); oadg_conv2d_dgrad_s2_nhwc_bf16:
# OADG_LS2(TB, PO); wgrad_launch: conv_wgrad256_kernel, conv_wgrad_kernel<1 | 2>, each also followed by
# wgrad_reduce_kernel ('(+reduce)'); oadg_conv2d_wgrad_multi.  prep_weights_kernel runs for the stride-2 class filters
# (hip_conv.prepared) and is audited by the wrapper on the way.  The remaining kernels of conv_mfma.hip prepare weights
# or consume partials (prep_weights_multi / _bwd / _bwd_parts / _bwd_parts_multi): they belong to the BN-fold chain the
# audited steps of tests/test_conv_audit.py gate at parameter level, not to this suite.
DISPATCH = (
    {'conv_igemm_kernel<%d, %s, %s>' % (tb, po, ns) for tb in (64, 128) for po in ('false', 'true')
     for ns in ('1, false', '1, true', '2, false')} |
    {'conv_igemm256_kernel<%s, %d>' % (po, nw) for po in ('false', 'true') for nw in (1, 2)} |
    {'conv_pw_stream_kernel<%d, %s, %s, %s>' % (c, 'true' if r else 'false', 'true' if m else 'false', 'true' if b else 'false')
     for c in STREAM for r, m, b in STREAM_FORMS} |
    {'conv_igemm_s2_kernel<%d, %s>' % (tb, po) for tb in (64, 128) for po in ('false', 'true')} |
    {k + s for k in ('conv_wgrad256_kernel', 'conv_wgrad_kernel<1>', 'conv_wgrad_kernel<2>') for s in ('', ' (+reduce)')} |
    {'conv_wgrad256_multi_kernel', 'prep_weights_kernel'} |
    {'n16_%s_kernel<%d>' % (k, c) for k in ('fwd', 'dgrad', 'wgrad') for c in (128, 256)} |
    {'bottleneck_frozen_kernel', 'bottleneck_frozen_first_kernel', 'stem_conv7x7s2_kernel'}
)


@pytest.mark.gpu
def test_zz_union_of_audited_instantiations_is_the_dispatch_table(dev):
    """runs last in this module: every entry of DISPATCH was launched under the auditor by the tests above, and nothing
    else was.  No combination of DISPATCH is unreachable from the Python entry points."""
    print('audited instantiations:', sorted(_SEEN))
    assert _SEEN == DISPATCH, (sorted(DISPATCH - _SEEN), sorted(_SEEN - DISPATCH))


def test_dispatch_table_size_and_case_names():
    """12 + 4 + 24 + 4 + 6 + 2 + 6 + 3 entries; every case names an entry"""
    assert len(DISPATCH) == 61
    named = {c[-1] for c in FWD_64 + FWD_128 + FWD_256} | {c[-1] for C in STREAM for c in stream_cases(C)} | \
        {c[-1] for c in S2_CASES} | {c[10] for c in WG_CASES}
    assert named <= DISPATCH, named - DISPATCH
    assert {n for n in DISPATCH if n.startswith(('conv_igemm', 'conv_pw'))} <= named
    # the auditor's tile rule is conv_launch's: 64-wide on every small map, 128-wide from 257 tiles
    for case in FWD_64 + FWD_128:
        N, C, H, W, K, R, stride, pad, dil = case[1]
        Ho, Wo = out_hw(H, W, R, stride, pad, dil)
        assert ('<%d,' % CA.tile_width(N * Ho * Wo, K)) in case[-1], case[0]
    assert CA.tile_width(256 * 128, 128) == 64 and CA.tile_width(256 * 128 + 1, 128) == 128 and CA.tile_width(10 ** 6, 192) == 64


# -------------------------------------------------------------------------------------------------------- CPU self-tests
CPU = torch.device('cpu')


def conv_f32(x, w, bias, stride, pad, dil, reverse=False, drop=None):
    """fp32 restatement of an implicit-GEMM convolution: per-tap, per-64-channel-chunk fp32 GEMMs accumulated in fp32, in
    tap-major order or reversed; ``drop`` = (pixel index, k, tap, channel): that one product never accumulated"""
    N, C, H, W = x.shape
    K, _, R, S_ = w.shape
    Ho, Wo = out_hw(H, W, R, stride, pad, dil)
    xf = x.float().permute(0, 2, 3, 1)
    acc = torch.zeros((N * Ho * Wo, K), dtype=torch.float32)
    steps = [((i, j), v, c0) for (i, j), v in CA._taps(xf, R, S_, stride, pad, dil, Ho, Wo) for c0 in range(0, C, 64)]
    for (i, j), v, c0 in (reversed(steps) if reverse else steps):
        m = v.reshape(-1, C)[:, c0:c0 + 64]
        wk = w.float()[:, c0:c0 + 64, i, j].t().clone()
        acc = acc + m @ wk
        if drop is not None and drop[2] == (i, j) and c0 <= drop[3] < c0 + 64:
            acc[drop[0], drop[1]] -= m[drop[0], drop[3] - c0] * wk[drop[3] - c0, drop[1]]
    if bias is not None:
        acc = acc + bias.float()
    return acc.view(N, Ho, Wo, K).double()


SELF_GEO = (2, 64, 9, 11, 128, 3, 1, 1, 1)


def _self_case(res=None, relu=False):
    x, w, b, r, _, _ = fwd_operands(CPU, SELF_GEO, res, None, 'int')
    yr, S, first, live = CA.forward_exact(x, w, b, r, 1, 1, 1, relu, res_up=False)
    assert float(S.max()) < CA.EXACT_LIMIT
    return x, w, b, r, yr, first, live


def test_bit_pattern_roundings_against_torch_and_each_other():
    t = torch.arange(-70000, 70001, dtype=torch.float64)
    assert torch.equal(CA.bf16_rne(t), t.float().to(torch.bfloat16).double())
    down, up = CA.bf16_ties(t)
    assert down > 100 and up > 100
    assert int((CA.bf16_half_away(t) != CA.bf16_rne(t)).sum()) == down          # exactly the ties RNE rounds down
    assert int((CA.bf16_trunc(t) != CA.bf16_rne(t)).sum()) > up
    with pytest.raises(AssertionError):
        CA.bf16_rne(torch.tensor([2.0 ** 24 + 1.0], dtype=torch.float64))      # not an fp32 value: outside the regime


def test_exact_check_accepts_two_summation_orders():
    x, w, b, r, yr, first, live = _self_case()
    A = CA.Auditor()
    for rev in (False, True):
        acc = conv_f32(x, w, b, 1, 1, 1, reverse=rev)
        assert A.exact('fp32 restatement', x.shape, CA.bf16_rne(acc), yr)
    assert not A.failures


def test_exact_check_rejects_truncation_and_round_half_away():
    x, w, b, r, yr, first, live = _self_case()
    down, up = CA.bf16_ties(first, live)
    assert down >= 100 and up >= 100, (down, up)
    acc = conv_f32(x, w, b, 1, 1, 1)
    for bad in (CA.bf16_trunc(acc), CA.bf16_half_away(acc)):
        A = CA.Auditor()
        assert not A.exact('fp32 restatement', x.shape, bad, yr)
        assert A.failures


def test_exact_check_rejects_one_dropped_product_in_a_corner_pixel():
    x, w, b, r, yr, first, live = _self_case()
    last = 2 * 9 * 11 - 1                    # the bottom-right pixel of the second image; its centre tap reads x[1, :, 8, 10]
    flat = first.reshape(-1, 128)
    # an output below 128 in magnitude: with or without the product (|x w| <= 32) it is stored without rounding
    k = int((flat[last].abs() < 128).nonzero()[0])
    c = int(((x[1, :, 8, 10].float() != 0) & (w[k, :, 1, 1].float() != 0)).nonzero()[0])
    acc = conv_f32(x, w, b, 1, 1, 1, drop=(last, k, (1, 1), c))
    assert int((acc != first).sum()) == 1
    A = CA.Auditor()
    assert not A.exact('fp32 restatement', x.shape, CA.bf16_rne(acc), yr)
    assert int((CA.bf16_rne(acc) != yr).sum()) == 1 and A.failures
    # (for scale: the same element under the auditor's bound RHO |r| + GAMMA S)
    _, bnd = CA.forward_expect(x, w, b, None, 1, 1, 1, False)
    print('dropped product %g at output %g: err / bound %.3f' % (
        float(x[1, c, 8, 10]) * float(w[k, c, 1, 1]), float(flat[last, k]), CA.ratio(CA.bf16_rne(acc), first, bnd)[0]))


def test_exact_check_rejects_a_single_rounding_where_the_contract_has_two():
    x, w, b, r, yr, first, live = _self_case(res='same', relu=True)
    acc = conv_f32(x, w, b, 1, 1, 1)
    two = CA.bf16_rne((CA.bf16_rne(acc) + CA._nhwc64(r)).clamp_min(0))
    one = CA.bf16_rne((acc + CA._nhwc64(r)).clamp_min(0))
    A = CA.Auditor()
    assert A.exact('fp32 restatement', x.shape, two, yr) and not A.failures
    assert not A.exact('fp32 restatement', x.shape, one, yr)
    print('single rounding differs at %d of %d elements' % (int((one != yr).sum()), yr.numel()))


def test_exact_check_rejects_a_split_partial_left_at_zero_and_one_left_unwritten():
    geo = (1, 128, 49, 43, 128, 1, 1, 0, 1)          # 33 chunks, 8 splits of 5: split 6 owns 3, split 7 none
    x, gy = wg_operands(CPU, geo, 'int')
    splits, pix = 8, 5 * 64
    ref, S = CA.wgrad_parts_exact(x, gy, 1, 1, 1, 0, 1, splits, pix)
    assert float(S.max()) < CA.EXACT_LIMIT
    dw, _ = CA.wgrad_ref(x, gy, 1, 1, 1, 0, 1)
    assert torch.equal(ref.sum(0).view(128, 128), dw.view(128, 128))
    assert float(ref[7].abs().max()) == 0 and float(ref[6].abs().max()) > 0
    good = ref.float()
    A = CA.Auditor()
    assert all(A.exact('fp32 restatement', x.shape, good[s], ref[s], check='split partial') for s in range(splits))
    # a partial left at zero whose pixels another split took over: the SUM over the splits is still right
    moved = good.clone()
    moved[2] += moved[6]
    moved[6] = 0
    assert torch.equal(moved.double().sum(0), ref.sum(0))
    B = CA.Auditor()
    assert [B.exact('fp32 restatement', x.shape, moved[s], ref[s], check='split partial') for s in range(splits)] == \
        [True, True, False, True, True, True, False, True]
    # the empty split left unwritten (whatever the workspace held)
    stale = good.clone()
    stale[7] = 3.0
    C_ = CA.Auditor()
    assert not C_.exact('fp32 restatement', x.shape, stale[7], ref[7], check='split partial') and C_.failures


CPU_FWD = FWD_64 + FWD_128 + FWD_256 + [stream_cases(C)[2] for C in sorted(STREAM)] + stream_cases(256)[-2:]


@pytest.mark.parametrize('case', CPU_FWD, ids=['%s %s' % (c[-1], c[0]) for c in CPU_FWD])
def test_integer_regime_conditions_hold_for_the_named_forward_cases(case):
    """S < 2^24 and the tie counts for every named forward case, on the CPU draw of the same operand recipe (the GPU tests
    assert them again on theirs): the streaming kernel's ranges depend on C and K only - one form per C, and the res_up pair"""
    cid, geo, variant, res, mask, bout, colsum, relu, name = case
    x, w, b, r, m, mb = fwd_operands(CPU, geo, res, mask, 'int')
    yr, S, first, live = CA.forward_exact(x, w, b, r, geo[6], geo[7], geo[8], relu, m, mb, res == 'up')
    ties, n_live = CA.bf16_ties(first, live), int(live.sum())
    print('%s: max S %d, %d live outputs, %.1f %% inexact in bf16, ties %d down / %d up' % (
        cid, int(S.max()), n_live, 100.0 * float((CA.bf16_rne(first) != first)[live].double().mean()) if n_live else 0.0, *ties))
    assert_regime(S, ties, n_live, cid)


def test_integer_regime_conditions_hold_for_the_other_families():
    """stride-2 data gradients, weight gradients (S only: fp32 outputs), narrow head ranges, the frozen block's three
    stages and the stem, on the CPU"""
    tally = Tally()
    for case in S2_CASES:
        cid, N, C, H, W, K, R, acc, mask, colsum, name = case
        gy, w, a, m, mb = s2_operands(CPU, case, 'int')
        yr, S, first, live = CA.dgrad_s2_exact(gy, w.to(torch.bfloat16), H, W, 1 if R == 3 else 0, a, m, mb)
        ties = CA.bf16_ties(first, live)
        print('%s: max S %d, ties %d / %d of %d' % (cid, int(S.max()), ties[0], ties[1], int(live.sum())))
        assert_regime(S, ties, int(live.sum()), cid)
        tally.add(ties, int(live.sum()))
    tally.check()
    for case in WG_CASES[:8]:
        geo = case[1:10]
        x, gy = wg_operands(CPU, geo, 'int')
        _, S = CA.wgrad_ref(x, gy, geo[5], geo[5], geo[6], geo[7], geo[8])
        assert float(S.max()) < CA.EXACT_LIMIT
    for case in WG_CASES[8:]:                  # (the 256-tile shapes: S <= P * 8 * 8 without computing it)
        N, C, H, W, K, R, stride, pad, dil = case[1:10]
        Ho, Wo = out_hw(H, W, R, stride, pad, dil)
        assert N * Ho * Wo * 64 < CA.EXACT_LIMIT
    g = _gen(CPU, 5)
    x, w = _ints((2, 3, 5, 6), 16, g, CPU).to(torch.bfloat16), _ints((64, 3, 7, 7), 8, g, CPU).to(torch.bfloat16)
    _, S, _, _ = CA.forward_exact(x, w, None, None, 2, 3, 1, False)
    assert float(S.max()) < CA.EXACT_LIMIT
    assert 367 * 64 * 16 < CA.EXACT_LIMIT and 256 * 16 * 8 + 64 < CA.EXACT_LIMIT      # the narrow head's worst cases


def test_frozen_block_integer_chain_stays_exact_on_the_cpu():
    """ternary / sparse weights keep S below 2^24 at all three stages of the frozen block, and the rounded chain holds
    enough ties at its last rounding"""
    for first in (False, True):
        g = _gen(CPU, 3 + int(first))
        cin = 64 if first else 256
        shapes = [(64, cin, 1, 1), (64, 64, 3, 3), (256, 64, 1, 1)] + ([(256, 64, 1, 1)] if first else [])
        ws = [(_ints(s, 1, g, CPU) * (torch.rand(s, generator=g) < d)).to(torch.bfloat16)
              for s, d in zip(shapes, (1.0, 0.25, 0.5, 1.0))]
        bs = [_ints((s[0],), 16, g, CPU) for s in shapes]
        x = _ints((3, cin, 9, 9), 8, g, CPU).to(torch.bfloat16)
        yr, Ss, firsts, live = CA.frozen_block_exact(x, ws, bs, first)
        t3 = CA.bf16_rne(firsts[2]) + (CA._nhwc64(x) if not first else
                                      CA.bf16_rne(CA.conv_ref(x, ws[3], 1, 0, 1)[0] + bs[3].double()))
        ties = CA.bf16_ties(t3, live)
        print('first=%s: max S per stage %s, ties %s of %d live' % (first, [int(S.max()) for S in Ss], ties, int(live.sum())))
        assert max(float(S.max()) for S in Ss) < CA.EXACT_LIMIT
        assert ties[0] >= 100 and ties[1] >= 100
        # the auditor's bound accepts the exact chain (the two references agree)
        r, b = CA.frozen_block_expect(x, ws, bs, first)
        assert CA.ratio(yr, r, b)[0] <= 1.0
