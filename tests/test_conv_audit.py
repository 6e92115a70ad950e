"""Elementwise fp64 audit of every convolution launch of a real training step (tests/conv_audit.py), plus CPU self-tests
showing that the auditor's reference and bound reject subtly wrong kernels.

GPU tests (``-m gpu``): three workloads on the deferred path TrainEngine._step takes; each asserts that no audited value
exceeds its bound, that every wrapper expected for the network saw a call, and that the set of audited kernel
instantiations equals the list written here (a launch routed around the auditor, or a new instantiation, fails the test).
"""
import pytest
import torch

import conv_audit as CA
from audit_workload import DC5_CFG, R50_CFG, audited_step


# ------------------------------------------------------------------------------------------- CPU self-tests of the checker
def _bf16(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def _rounded(r_nhwc):
    """a correctly rounded bf16 output of the fp64 value"""
    return r_nhwc.to(torch.bfloat16).to(torch.float64)


def _worst(o, ref, b):
    return CA.ratio(o, ref, b)[0]


def _conv_case(C=128, K=64, R=3, stride=1, pad=1, H=9, W=11, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = _bf16((2, C, H, W), g)
    w = _bf16((K, C, R, R), g, 0.05)
    bias = torch.randn(K, generator=g) * 0.1
    r, b = CA.forward_expect(x, w, bias, None, stride, pad, 1, True)
    return x, w, bias, r, b


def test_checker_accepts_correct_rounding_and_rejects_a_moved_element():
    x, w, bias, r, b = _conv_case()
    o = _rounded(r)
    assert _worst(o, r, b) <= 1.0
    o2 = o.clone()
    i = int((r.abs() > 0.1).reshape(-1).nonzero()[0])
    o2.view(-1)[i] += 2 * b.view(-1)[i]
    assert _worst(o2, r, b) > 1.0


def test_checker_rejects_edge_clamped_halo_row():
    x, w, bias, r, b = _conv_case()
    # a kernel that reads the top halo row from the image's first row instead of the zero padding
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    xp[:, :, 0, 1:-1] = x.double()[:, :, 0]
    bad = torch.nn.functional.conv2d(xp, w.double()) + bias.double().view(1, -1, 1, 1)
    o = _rounded(bad.clamp_min(0).permute(0, 2, 3, 1))
    assert _worst(o, r, b) > 1.0


def test_checker_rejects_one_dropped_channel_chunk_of_one_tap():
    x, w, bias, r, b = _conv_case(C=128)
    w2 = w.clone()
    w2[:, 64:128, 2, 0] = 0          # the second 64-channel chunk of tap (2, 0) never accumulated
    bad, _ = CA.forward_expect(x, w2, bias, None, 1, 1, 1, True)
    assert _worst(_rounded(bad), r, b) > 1.0


def test_checker_rejects_a_dropped_wgrad_split_partial():
    g = torch.Generator().manual_seed(1)
    x = _bf16((4, 64, 8, 8), g)
    gy = _bf16((4, 64, 8, 8), g)
    dw, S = CA.wgrad_ref(x, gy, 3, 3, 1, 1, 1)
    b = CA.bound(dw, S, 0.0)
    # four fp32 split partials over the images ([splits][K][C][R][S]: the sum over the splits does not depend on the
    # layout of one partial)
    parts = torch.stack([CA.wgrad_ref(x[i:i + 1], gy[i:i + 1], 3, 3, 1, 1, 1)[0].float() for i in range(4)])
    summed = parts.double().sum(0)
    assert _worst(summed, dw, b) <= 1.0
    assert _worst(parts[:3].double().sum(0), dw, b) > 1.0


def test_checker_rejects_one_flipped_mask_bit():
    g = torch.Generator().manual_seed(2)
    x = _bf16((2, 64, 6, 6), g)
    w = _bf16((64, 64, 1, 1), g, 0.1)
    m = _bf16((2, 64, 6, 6), g)
    bits = CA.pack_bits(CA._nhwc64(m) > 0)
    r, b = CA.forward_expect(x, w, None, None, 1, 0, 1, False, mask_bits=bits)
    o = _rounded(r)
    assert _worst(o, r, b) <= 1.0
    assert torch.equal(CA.unpack_bits(bits, r.shape), CA._nhwc64(m) > 0)
    # flip the bit of an element whose unmasked value is clearly non-zero
    r_all, _ = CA.forward_expect(x, w, None, None, 1, 0, 1, False)
    i = int(((r_all.abs() > 0.05) & (r != 0)).reshape(-1).nonzero()[0])
    bad = bits.clone()
    bad[i // 8] ^= 1 << (i % 8)
    r_bad, _ = CA.forward_expect(x, w, None, None, 1, 0, 1, False, mask_bits=bad)
    assert _worst(_rounded(r_bad), r, b) > 1.0


def test_checker_rejects_a_column_sum_missing_one_tile_row():
    x, w, bias, r, b = _conv_case()
    y = _rounded(r)
    cs, S = CA.colsum_expect(y)
    rows = y.reshape(-1, y.shape[-1]).float().split(64)          # per-64-pixel-tile partials of the stored output
    part = torch.stack([t.sum(0) for t in rows])
    assert _worst(part.double().sum(0), cs, CA.bound(cs, S, 0.0)) <= 1.0
    assert _worst(part[1:].double().sum(0), cs, CA.bound(cs, S, 0.0)) > 1.0


def test_checker_rejects_dgamma_without_its_mean_term():
    g = torch.Generator().manual_seed(3)
    K, C = 64, 32
    w = torch.randn((K, C, 3, 3), generator=g) * 0.05
    gamma, mean = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    var = torch.rand(K, generator=g) + 0.1
    dwf = torch.randn((K, C, 3, 3), generator=g, dtype=torch.float64)
    db = torch.randn(K, generator=g, dtype=torch.float64)
    dW, SdW, dg, Sdg = CA.bn_chain_expect(dwf, dwf.abs(), db, db.abs(), w, gamma, mean, var, 1e-5)
    inv = 1.0 / torch.sqrt(var.double() + 1e-5)
    good = ((dwf * w.double()).sum((1, 2, 3)).float() - db.float() * mean) * inv.float()
    no_mean = (dwf * w.double()).sum((1, 2, 3)).float() * inv.float()
    b = CA.bound(dg, Sdg, 0.0)
    assert _worst(good.double(), dg, b) <= 1.0
    assert _worst(no_mean.double(), dg, b) > 1.0
    assert _worst((dwf * (gamma.double() * inv).view(-1, 1, 1, 1)).float().double(), dW, CA.bound(dW, SdW, 0.0)) <= 1.0


@pytest.mark.parametrize('R', [3, 1])
def test_checker_rejects_stride2_class_on_the_wrong_parity(R):
    g = torch.Generator().manual_seed(4)
    N, C, K, H, W = 2, 64, 64, 10, 12
    w = _bf16((K, C, R, R), g, 0.1)
    gy = _bf16((N, K, H // 2, W // 2), g)
    pad = 1 if R == 3 else 0
    r, S = CA.dgrad_s2_ref(gy, w, H, W, pad)
    # the fp64 reference agrees with autograd's stride-2 data gradient
    xg = torch.zeros((N, C, H, W), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xg, w.double(), stride=2, padding=pad).backward(gy.double())
    assert torch.allclose(xg.grad.permute(0, 2, 3, 1), r, rtol=1e-12, atol=1e-12)
    b = CA.bound(r, S, CA.RHO)
    o = _rounded(r)
    assert _worst(o, r, b) <= 1.0
    bad = o.clone()
    if R == 3:
        bad[:, 0::2, 1::2] = o[:, 1::2, 0::2]          # class (1, 0) written on the (0, 1) grid
    else:
        bad[:, 1::2, 1::2] = o[:, 0::2, 0::2]          # the single class written on the odd grid
        bad[:, 0::2, 0::2] = 0
    assert _worst(bad, r, b) > 1.0


def test_s2_filters_decode_the_parity_class_layout():
    """the auditor's decoder of prep_weights_channel's wt_mode 2 layout, against that layout built independently"""
    g = torch.Generator().manual_seed(5)
    K, C = 64, 128
    w = _bf16((K, C, 3, 3), g)
    blocks = []
    for ph, pw in ((0, 0), (0, 1), (1, 0), (1, 1)):
        rs = [1] if ph == 0 else [2, 0]
        qs = [1] if pw == 0 else [2, 0]
        blocks.append(torch.stack([w[:, :, r, q].t() for r in rs for q in qs], 1))       # [C][taps][K]
    flat = torch.cat([b_.reshape(-1) for b_ in blocks])
    wt = flat.view(C, 3, 3, K).permute(0, 3, 1, 2)      # a channels_last [C, K, 3, 3] tensor over that memory
    assert torch.equal(CA.s2_filters(wt, K, C, 3), w)


def test_frozen_block_reference_matches_its_rounding_and_rejects_a_missed_rounding():
    g = torch.Generator().manual_seed(6)
    x = _bf16((1, 256, 6, 7), g).clamp_min(0)
    ws = [_bf16((64, 256, 1, 1), g, 0.06), _bf16((64, 64, 3, 3), g, 0.04), _bf16((256, 64, 1, 1), g, 0.1)]
    bs = [torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1, torch.randn(256, generator=g) * 0.1]
    r, b = CA.frozen_block_expect(x, ws, bs, False)
    # the kernel's arithmetic, with its roundings, through torch
    c = lambda t, w_, b_, p: torch.nn.functional.conv2d(t.double(), w_.double(), padding=p) + b_.double().view(1, -1, 1, 1)  # noqa: E731
    t1 = c(x, ws[0], bs[0], 0).clamp_min(0).to(torch.bfloat16)
    t2 = c(t1, ws[1], bs[1], 1).clamp_min(0).to(torch.bfloat16)
    t3 = c(t2, ws[2], bs[2], 0).to(torch.bfloat16).double()
    y = (t3 + x.double()).clamp_min(0).to(torch.bfloat16)
    assert _worst(CA._nhwc64(y), r, b) <= 1.0
    # conv2 without its bias: rejected
    t2b = (c(t1, ws[1], bs[1], 1) - bs[1].double().view(1, -1, 1, 1)).clamp_min(0).to(torch.bfloat16)
    yb = (c(t2b, ws[2], bs[2], 0).to(torch.bfloat16).double() + x.double()).clamp_min(0).to(torch.bfloat16)
    assert _worst(CA._nhwc64(yb), r, b) > 1.0


def test_residual_up2_reference_and_its_named_rounding():
    g = torch.Generator().manual_seed(7)
    x = _bf16((2, 64, 8, 10), g)
    w = _bf16((64, 64, 1, 1), g, 0.1)
    top = _bf16((2, 64, 4, 5), g)
    r, b = CA.forward_expect(x, w, None, top, 1, 0, 1, False, res_up=True)
    conv = torch.nn.functional.conv2d(x.double(), w.double())
    # finish_piece: bf16 tile, + bf16 residual, rounded again
    y = (conv.to(torch.bfloat16).double() + torch.nn.functional.interpolate(top.double(), scale_factor=2.0)).to(torch.bfloat16)
    assert _worst(CA._nhwc64(y), r, b) <= 1.0
    y_plain = conv.to(torch.bfloat16)             # the top-down add dropped
    assert _worst(CA._nhwc64(y_plain), r, b) > 1.0


@pytest.mark.parametrize('fused', [False, True])
def test_head_rows_map_to_rpn_cls_and_rpn_reg(fused):
    """check_params splits the RPN head's fp64 row gradients [rpn_cls; rpn_reg; zero padding] back onto the two modules
    (narrow head: 16 rows; fused head: one unbanked 1x1 convolution of 128 rows) and rejects rows taken one off"""
    g = torch.Generator().manual_seed(8)
    cls, reg = torch.nn.Conv2d(8, 3, 1), torch.nn.Conv2d(8, 12, 1)
    rows = 128 if fused else 16
    dw = torch.randn((rows, 8), generator=g, dtype=torch.float64)
    db = torch.randn(rows, generator=g, dtype=torch.float64)
    named = [('rpn_head.rpn_cls.weight', cls.weight), ('rpn_head.rpn_cls.bias', cls.bias),
             ('rpn_head.rpn_reg.weight', reg.weight), ('rpn_head.rpn_reg.bias', reg.bias)]
    for shift, ok in ((0, True), (1, False)):
        A = CA.Auditor()
        if fused:
            tok = object()          # (an unbanked weight is keyed by its weight-gradient token)
            A.params[id(tok)] = [tok, dw.view(rows, 8, 1, 1), dw.abs().view(rows, 8, 1, 1), db, db.abs(), 1]
        else:
            A.narrow = [dw, dw.abs(), db, db.abs()]
        cls.weight.grad = dw[shift:shift + 3].view(3, 8, 1, 1).float()
        cls.bias.grad = db[shift:shift + 3].float()
        reg.weight.grad = dw[3:15].view(12, 8, 1, 1).float()
        reg.bias.grad = db[3:15].float()
        assert A.check_params(named, [cls, reg]) == {n for n, _ in named}
        assert (not A.failures) == ok, A.failures


# ------------------------------------------------------------------------------------------------- GPU audited steps
# kernels every workload must reach through the audited wrappers
_COMMON = {
    'bias_relu_maxpool_kernel', 'stem_conv7x7s2_kernel', 'bottleneck_frozen_kernel', 'bottleneck_frozen_first_kernel',
    'prep_weights_multi_kernel',     # (the bank refresh after the audited step's optimizer step)
}

# the kernel instantiations each workload launches (spelt as hip_conv.kernel_name / rocprofv3 print them, the tile width
# of the 128-pixel family by conv_launch's rule - conv_audit.tile_width; the weight-gradient kernel that reduces its own
# splits carries ' (+reduce)')
EXPECTED = {
    'r50_fpn': {
        'bias_relu_maxpool_kernel',
        'bottleneck_frozen_first_kernel',
        'bottleneck_frozen_kernel',
        'colsum_reduce_kernel',
        'colsum_reduce_multi_kernel',
        'conv_igemm256_kernel<false, 2>',
        'conv_igemm256_kernel<true, 2>',
        'conv_igemm_kernel<128, false, 1, false>',
        'conv_igemm_kernel<128, false, 1, true>',
        'conv_igemm_kernel<128, false, 2, false>',
        'conv_igemm_kernel<128, true, 1, false>',
        'conv_igemm_kernel<128, true, 2, false>',
        'conv_igemm_kernel<64, false, 2, false>',       # (P5 / P6: 128-wide tiles would leave compute units idle)
        'conv_igemm_s2_kernel<128, true>',
        'conv_pw_stream_kernel<128, true, false, true>',
        'conv_pw_stream_kernel<128, true, true, false>',
        'conv_pw_stream_kernel<256, false, false, false>',
        'conv_pw_stream_kernel<256, true, false, false>',
        'conv_pw_stream_kernel<256, true, false, true>',
        'conv_pw_stream_kernel<256, true, true, false>',
        'conv_pw_stream_kernel<512, false, false, true>',
        'conv_pw_stream_kernel<512, false, true, false>',
        'conv_pw_stream_kernel<512, true, false, false>',
        'conv_pw_stream_kernel<512, true, false, true>',
        'conv_pw_stream_kernel<512, true, true, false>',
        'conv_wgrad256_kernel',
        'conv_wgrad256_multi_kernel',
        'conv_wgrad_kernel<1>',
        'conv_wgrad_kernel<2>',
        'fpn_topdown_bwd_kernel',
        'fpn_topdown_fwd_kernel',
        'n16_dgrad_kernel<256>',
        'n16_fwd_kernel<256>',
        'n16_wgrad_kernel<256>',
        'prep_weights_multi_kernel',
        'relu_bias_bwd_kernel',
        'stem_conv7x7s2_kernel',
    },
    'r101_dc5': {
        'bias_relu_maxpool_kernel',
        'prep_weights_kernel',          # (the fused RPN head's weights: built from rpn_cls / rpn_reg every step)
        'bottleneck_frozen_first_kernel',
        'bottleneck_frozen_kernel',
        'colsum_reduce_multi_kernel',
        'conv_igemm256_kernel<false, 2>',
        'conv_igemm_kernel<128, false, 1, false>',
        'conv_igemm_kernel<128, false, 1, true>',
        'conv_igemm_kernel<128, false, 2, false>',
        'conv_igemm_kernel<128, true, 1, false>',
        'conv_igemm_kernel<128, true, 1, true>',
        'conv_igemm_kernel<128, true, 2, false>',
        'conv_igemm_kernel<64, false, 1, false>',       # (the 46 x 80 maps: 115 pixel tiles x K / 128 <= 256 workgroups)
        'conv_igemm_kernel<64, false, 1, true>',
        'conv_igemm_kernel<64, false, 2, false>',
        'conv_igemm_kernel<64, true, 1, true>',
        'conv_igemm_kernel<64, true, 2, false>',
        'conv_igemm_s2_kernel<128, false>',
        'conv_igemm_s2_kernel<128, true>',
        'conv_pw_stream_kernel<512, true, false, true>',
        'conv_pw_stream_kernel<512, true, true, false>',
        'conv_wgrad256_kernel (+reduce)',
        'conv_wgrad256_multi_kernel',
        'conv_wgrad_kernel<1>',
        'conv_wgrad_kernel<2>',
        'prep_weights_multi_kernel',
        'relu_bias_bwd_kernel',
        'stem_conv7x7s2_kernel',
    },
    # (the ragged shape reaches conv_igemm_kernel<128, true, 1, true>: a 1x1 data gradient whose pixel count is no
    #  multiple of the streaming kernel's ranges, and no 512-channel streaming kernel with bits out)
    'r50_fpn_multiscale': {
        'bias_relu_maxpool_kernel',
        'bottleneck_frozen_first_kernel',
        'bottleneck_frozen_kernel',
        'colsum_reduce_kernel',
        'colsum_reduce_multi_kernel',
        'conv_igemm256_kernel<false, 2>',
        'conv_igemm256_kernel<true, 2>',
        'conv_igemm_kernel<128, false, 1, false>',
        'conv_igemm_kernel<128, false, 1, true>',
        'conv_igemm_kernel<128, false, 2, false>',
        'conv_igemm_kernel<128, true, 1, false>',
        'conv_igemm_kernel<128, true, 1, true>',
        'conv_igemm_kernel<128, true, 2, false>',
        'conv_igemm_kernel<64, false, 2, false>',
        'conv_igemm_kernel<64, true, 2, false>',
        'conv_igemm_s2_kernel<128, true>',
        'conv_pw_stream_kernel<128, true, false, true>',
        'conv_pw_stream_kernel<128, true, true, false>',
        'conv_pw_stream_kernel<256, false, false, false>',
        'conv_pw_stream_kernel<256, true, false, false>',
        'conv_pw_stream_kernel<256, true, false, true>',
        'conv_pw_stream_kernel<256, true, true, false>',
        'conv_pw_stream_kernel<512, false, false, true>',
        'conv_pw_stream_kernel<512, false, true, false>',
        'conv_pw_stream_kernel<512, true, false, false>',
        'conv_pw_stream_kernel<512, true, true, false>',
        'conv_wgrad256_kernel',
        'conv_wgrad256_multi_kernel',
        'conv_wgrad_kernel<1>',
        'conv_wgrad_kernel<2>',
        'fpn_topdown_bwd_kernel',
        'fpn_topdown_fwd_kernel',
        'n16_dgrad_kernel<256>',
        'n16_fwd_kernel<256>',
        'n16_wgrad_kernel<256>',
        'prep_weights_multi_kernel',
        'relu_bias_bwd_kernel',
        'stem_conv7x7s2_kernel',
    },
}

WRAPPERS = {
    'r50_fpn': {'conv_forward', 'conv_dgrad_s2', 'conv_wgrad_parts', 'wgrad_multi', 'relu_bias_bwd', '_colsum',
                'resolve_colsum', 'flush_colsums', 'frozen_bottleneck', '_PrepWeights.forward', '_PrepWeights.backward',
                '_Bank.refresh', '_Conv2dMFMA.backward', '_NarrowHead.forward', '_NarrowHead.backward', 'stem_conv',
                'bias_relu_maxpool', '_FpnTopDown.forward', '_FpnTopDown.backward',
                '_Conv2dMFMA.backward res_up'},      # (the FPN top-down add fused into a lateral convolution: its backward)
}
WRAPPERS['r50_fpn_multiscale'] = WRAPPERS['r50_fpn']
# no FPN, no narrow head; the 2048 -> 2048 RPN convolution (shared by nothing, too wide for split partials) reduces its own
# weight gradient (conv_wgrad) and hands it to the BN-fold chain rule in bf16
WRAPPERS['r101_dc5'] = WRAPPERS['r50_fpn'] - {'_NarrowHead.forward', '_NarrowHead.backward', '_FpnTopDown.forward',
                                              '_FpnTopDown.backward', 'resolve_colsum',
                                              '_Conv2dMFMA.backward res_up'} | {'conv_wgrad'}


def _audited_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size, key):
    A = CA.Auditor()
    checked = []

    def on_begin():
        A.params.clear()
        A.bf16_handover.clear()
        A.narrow = None

    def on_end_backward(det):
        head = det.rpn_head
        checked.append(A.check_params(list(det.named_parameters()), [head.rpn_cls, head.rpn_reg]))

    out, det, wall = audited_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size,
                                  lambda mp, det: A.install(mp), on_begin, on_end_backward)
    A.print_table('%s (audited step %.1f s)' % (key, wall))
    print('worst err / bound: %.4f' % A.worst())
    return A, det, checked[-1], wall


def _assert_audit(A, det, checked, key, expected_params):
    assert not A.failures, A.failures[:10]
    missing = WRAPPERS[key] - set(A.wrappers)
    assert not missing, missing
    want = [n for n, p in det.named_parameters() if p.requires_grad and expected_params(n)]
    assert want and not set(want) - checked, sorted(set(want) - checked)[:10]
    kernels = A.kernels         # (launched in the audited step: not the bank's tensors from the step before)
    exp = EXPECTED[key]
    print('audited instantiations:', sorted(kernels))
    assert _COMMON <= kernels, _COMMON - kernels
    assert kernels == exp, (sorted(kernels - exp), sorted(exp - kernels))


@pytest.mark.gpu
def test_audit_config1_r50_fpn_bench_step(dev, monkeypatch):
    """configs[1] as bench.py builds it: R50-FPN, 4 images x 2 views at 1024 x 2048, bf16, device OA-Mix pipeline; the
    SECOND step is audited so that the bank refresh of the first step's optimizer feeds the audited forward pass."""
    A, det, checked, wall = _audited_step(dev, monkeypatch, R50_CFG, 4, 1024, 2048, 20, 8, (24, 400), 'r50_fpn')
    _assert_audit(A, det, checked, 'r50_fpn', lambda n: n.startswith(('backbone.', 'neck.', 'rpn_head.')))


@pytest.mark.gpu
def test_audit_config3_r101_dc5(dev, monkeypatch):
    """configs[3]: R101-DC5, 2 images at 736 x 1280 - dilated layer4, one stride-16 RPN level, no FPN"""
    A, det, checked, wall = _audited_step(dev, monkeypatch, DC5_CFG, 2, 736, 1280, 12, 7, (24, 300), 'r101_dc5')
    # (rpn_cls / rpn_reg: 15 + 60 output channels, too many for the narrow head - one 1x1 convolution zero-padded to 128
    #  output channels, prepared by its own launch every step: dense_heads.py _fused_head_params)
    _assert_audit(A, det, checked, 'r101_dc5', lambda n: n.startswith(('backbone.', 'rpn_head.')))


@pytest.mark.gpu
def test_audit_multiscale_800x1600(dev, monkeypatch):
    """A shape of the multi-scale Resize range (faster_rcnn_r50_fpn_1x_cityscapes_oadg_multiscale.py: short side 800 - 1024,
    padded to 32): 2 images at 800 x 1600, 4 views.  Pixel counts the power-of-two benchmark shape never has: M = 80000 at
    stride 8 (a multiple of 64, not of 256), 20000 at stride 16, 5000 at stride 32 (P5 / layer4 at 25 x 50) and 1300 on the RPN's P6 (13 x 25, P5 subsampled): multiples of
    neither 64 nor 256 - partial pixel tiles in the forward / data-gradient kernels, partial pixel K-tiles in the weight
    gradients.  The 1 x 1 data gradient of layer3's conv3 (M = 20000, mask bits) goes to conv_igemm_kernel<128, true, 1,
    true> instead of the streaming kernel it takes at the benchmark shape."""
    A, det, checked, wall = _audited_step(dev, monkeypatch, R50_CFG, 2, 800, 1600, 12, 8, (24, 300), 'r50_fpn_multiscale')
    _assert_audit(A, det, checked, 'r50_fpn_multiscale',
                  lambda n: n.startswith(('backbone.', 'neck.', 'rpn_head.rpn_conv.')))
