"""The fp32 launch auditor (tests/f32_audit.py): every launch of the fp32 parity step against float64.

CPU: the references against torch's float64 convolution with autograd over the stress geometry list, one planted error per
kernel loop that the bound at GAMMA_F32 must reject, the numerical plant (one long float32 chain instead of the kernels'
blocked sums), the constants against the a-priori bound of the documented summation tree.

GPU: three audited fp32 steps (what ``bench.py --dtype fp32`` builds) under this auditor, head_audit.Auditor and
target_audit.Auditor together - no failure, no library convolution, no launch label that none of the three verified - and
direct ``conv2d_f32`` calls at the edges a step does not reach, judged by the same references and bound.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import f32_audit as FA  # noqa: E402
import head_audit as HA  # noqa: E402
import target_audit as TA  # noqa: E402
from audit_workload import DC5_CFG, R50_CFG, audited_step  # noqa: E402
from test_head_audit import BORDERLINE_CAP  # noqa: E402
from test_target_audit import CHECKED, LABEL_OF  # noqa: E402
from test_target_audit import WRAPPERS as TARGET_WRAPPERS  # noqa: E402

# ------------------------------------------------------------------------------------------------- the stress geometries
# (name, N, C, H, W, K, R, S, stride, pad, dil)
GEOMETRIES = [
    # channel counts: C = 4 only; C = 3 / 5 (padded to 4 / 8); C = 36 / 68 (a last 32-chunk with one live 16-byte piece);
    # K = 1, 3, 63, 64, 65 (a second 64-channel tile with one live column), 15, 60
    ('C4 K1', 1, 4, 9, 11, 1, 3, 3, 1, 1, 1),
    ('C3 K3', 2, 3, 13, 10, 3, 3, 3, 1, 1, 1),
    ('C5 K63', 1, 5, 8, 9, 63, 1, 1, 1, 0, 1),
    ('C36 K64', 1, 36, 10, 12, 64, 3, 3, 1, 1, 1),
    ('C68 K65', 1, 68, 7, 9, 65, 3, 3, 1, 1, 1),
    ('C256 K15', 1, 256, 9, 9, 15, 1, 1, 1, 0, 1),
    ('C256 K60', 1, 256, 9, 9, 60, 1, 1, 1, 0, 1),
    # pixel counts: M = 1, 127, 128, 129, and one above 2^16 that is no multiple of 128
    ('M1', 1, 8, 1, 1, 8, 1, 1, 1, 0, 1),
    ('M127', 1, 8, 1, 127, 8, 1, 1, 1, 0, 1),
    ('M128', 1, 8, 8, 16, 8, 3, 3, 1, 1, 1),
    ('M129', 1, 8, 3, 43, 8, 3, 3, 1, 1, 1),
    ('M65884', 2, 8, 181, 182, 16, 3, 3, 1, 1, 1),
    # stride 2 with even and odd sizes: 1x1 / pad 0 (whole parity classes of dx receive nothing; even: the last row / column
    # is never read), 3x3 / pad 1, 7x7 / pad 3; stride 3
    ('s2 1x1 even', 1, 16, 8, 10, 32, 1, 1, 2, 0, 1),
    ('s2 1x1 odd', 1, 16, 9, 11, 32, 1, 1, 2, 0, 1),
    ('s2 3x3 even', 1, 16, 8, 10, 32, 3, 3, 2, 1, 1),
    ('s2 3x3 odd', 1, 16, 9, 11, 32, 3, 3, 2, 1, 1),
    ('s2 7x7 even', 1, 3, 20, 22, 64, 7, 7, 2, 3, 1),
    ('s2 7x7 odd', 1, 3, 21, 23, 64, 7, 7, 2, 3, 1),
    ('s3 3x3', 1, 8, 11, 14, 8, 3, 3, 3, 1, 1),
    # dilation 2 / pad 2, dilation 3 with a padding larger than the image
    ('d2 p2', 1, 32, 9, 12, 32, 3, 3, 1, 2, 2),
    ('d3 p6 > image', 1, 8, 4, 5, 8, 3, 3, 1, 6, 3),
    # non-square filters with equal padding (the kernels take R and S separately)
    ('1x3', 1, 8, 7, 9, 8, 1, 3, 1, 1, 1),
    ('3x1', 1, 8, 7, 9, 8, 3, 1, 1, 1, 1),
]


def _geo(name):
    return GEOMETRIES[[g[0] for g in GEOMETRIES].index(name)]


def _operands(geo, seed=0, relu=False, positive=False, bias=True, device='cpu'):
    """(x, w, bias, gy) float32 from a seeded generator; ``relu``: x as a ReLU leaves it; ``positive``: everything
    non-negative (same-signed products in all three reductions)"""
    _, N, C, H, W, K, R, S, stride, pad, dil = geo
    g = torch.Generator().manual_seed(1000 * seed + N + C + H + W + K + R + S + stride + pad + dil)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, S, generator=g) / math.sqrt(C * R * S)
    b = torch.randn(K, generator=g) if bias else None
    Ho, Wo = FA.out_size(H, R, stride, pad, dil), FA.out_size(W, S, stride, pad, dil)
    gy = torch.randn(N, K, Ho, Wo, generator=g)
    if relu or positive:
        x = x.clamp_min(0)
    if positive:
        w, gy = w.abs(), gy.abs()
    return tuple(t.to(device) if t is not None else None for t in (x, w, b, gy))


def _f32(r):
    """the correctly rounded float32 of a float64 value, as float64"""
    return r.to(torch.float32).to(torch.float64)


def _worst(o, r, S, gamma):
    return FA.ratio(o, r, FA.bound(S, gamma))[0]


# ---------------------------------------------------------------------------------------- references against torch (CPU)
@pytest.mark.parametrize('geo', GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_references_match_torch_float64_convolution_with_autograd(geo):
    _, N, C, H, W, K, R, S, stride, pad, dil = geo
    x, w, b, gy = _operands(geo)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.conv2d(xr, wr, br, stride, pad, dil)
    (yr * gy.double()).sum().backward()

    def same(a, ref, S_):
        # float64 rounding of sums of S_: the two sides add the same terms in different orders
        assert a.shape == ref.shape and bool(((a - ref).abs() <= 1e-13 * S_ + 1e-300).all())
        assert bool((S_ >= a.abs() * (1 - 1e-12)).all())

    r, Sa = FA.conv_ref(x, w, stride, pad, dil)
    same(r + b.double(), yr.detach().permute(0, 2, 3, 1), Sa + b.double().abs())
    same(FA.gather_conv(x, w, stride, pad, dil, r.shape[1], r.shape[2]), r, Sa)
    dx, Sx = FA.dgrad_ref(gy, w, H, W, stride, pad, dil)
    same(dx, xr.grad.permute(0, 2, 3, 1), Sx)
    same(FA.gather_dgrad(gy, w, H, W, stride, pad, dil), dx, Sx)
    dw, Sw = FA.wgrad_ref(x, gy, R, S, stride, pad, dil)
    same(dw, wr.grad, Sw)
    g64 = gy.double().permute(0, 2, 3, 1).reshape(-1, K)
    same(g64.sum(0), br.grad, g64.abs().sum(0))


def test_strided_1x1_data_gradient_leaves_whole_parity_classes_exactly_zero():
    """stride 2, 1x1, pad 0: only the even rows / columns of dx receive a tap - S is zero elsewhere, so the bound there is
    ALPHA; with even sizes the last row and column are never read"""
    x, w, b, gy = _operands(_geo('s2 1x1 even'))
    dx, S = FA.dgrad_ref(gy, w, 8, 10, 2, 0, 1)
    assert bool((S[:, 1::2] == 0).all()) and bool((S[:, :, 1::2] == 0).all()) and bool((S[:, ::2, ::2] > 0).all())
    assert bool((dx[:, 7] == 0).all()) and bool((dx[:, :, 9] == 0).all())
    o = _f32(dx)
    assert _worst(o, dx, S, FA.GAMMA_F32_CONV) <= 1.0
    o[0, 1, 1, 0] = 1e-20                                            # a stale value in a class that receives nothing
    assert _worst(o, dx, S, FA.GAMMA_F32_CONV) > 1.0


def test_split_plan_restated_and_the_empty_trailing_splits_of_the_ragged_head_gradient():
    # the rpn_cls weight gradient at P = 300,000: 512 splits of 592 pixels, and 511 x 592 > P
    assert FA.wgrad_plan(1, 500, 600, 256, 4, 1, 1) == (512, 592) and 511 * 592 > 300000
    assert FA.empty_trailing_splits(300000, 512, 592) == 5
    assert FA.wgrad_plan(8, 256, 512, 256, 4, 1, 1) == (512, 2048)      # the bench step's P2 level
    assert FA.wgrad_plan(4, 46, 80, 2048, 2048, 3, 3) == (1, 14720)     # DC5: one split
    assert FA.wgrad_plan(1, 1, 524389, 32, 4, 1, 1)[0] == 1024          # the cap
    assert FA.empty_trailing_splits(1024, 2, 512) == 0


# ------------------------------------------------------------------------------------------------- planted errors (CPU)
def _fwd(geo, **kw):
    x, w, b, gy = _operands(geo, **kw)
    r, S = FA.conv_ref(x, w, *geo[8:11])
    return x, w, b, gy, r + b.double(), S + b.double().abs()


def test_bound_rejects_a_dropped_tap_at_the_image_border():
    geo = _geo('C36 K64')
    x, w, b, gy, r, S = _fwd(geo)
    assert _worst(_f32(r), r, S, FA.GAMMA_F32_CONV) <= 1.0
    xb = x.clone()
    xb[:, :, -1] = 0                                                 # `hi < H - 1`: the bottom row's taps never gathered
    bad = FA.conv_ref(xb, w, 1, 1, 1)[0] + b.double()
    assert bool((bad[:, :-2] == r[:, :-2]).all())                    # only the border rows differ
    assert _worst(_f32(bad), r, S, FA.GAMMA_F32_CONV) > 1.0


def test_bound_rejects_taps_gathered_with_dilation_and_stride_swapped():
    for name in ('s2 3x3 odd', 'd2 p2'):
        geo = _geo(name)
        x, w, b, gy, r, S = _fwd(geo)
        stride, pad, dil = geo[8:11]
        good = FA.gather_conv(x, w, stride, pad, dil, r.shape[1], r.shape[2]) + b.double()
        bad = FA.gather_conv(x, w, stride, pad, dil, r.shape[1], r.shape[2], plant='dil and stride swapped') + b.double()
        assert _worst(_f32(good), r, S, FA.GAMMA_F32_CONV) <= 1.0
        assert _worst(_f32(bad), r, S, FA.GAMMA_F32_CONV) > 1.0


def test_bound_rejects_a_transposed_gather_without_the_divisibility_test():
    for name in ('s2 3x3 even', 's2 1x1 odd', 's3 3x3'):
        geo = _geo(name)
        _, N, C, H, W, K, R, S_, stride, pad, dil = geo
        x, w, b, gy = _operands(geo)
        dx, S = FA.dgrad_ref(gy, w, H, W, stride, pad, dil)
        assert _worst(_f32(FA.gather_dgrad(gy, w, H, W, stride, pad, dil)), dx, S, FA.GAMMA_F32_CONV) <= 1.0
        bad = FA.gather_dgrad(gy, w, H, W, stride, pad, dil, plant='no divisibility test')
        assert _worst(_f32(bad), dx, S, FA.GAMMA_F32_CONV) > 1.0


def test_bound_rejects_an_ignored_last_channel_chunk():
    for name, live in (('C36 K64', 32), ('C68 K65', 64)):
        geo = _geo(name)
        x, w, b, gy, r, S = _fwd(geo)
        bad = FA.conv_ref(x[:, :live], w[:, :live], *geo[8:11])[0] + b.double()
        assert _worst(_f32(bad), r, S, FA.GAMMA_F32_CONV) > 1.0


def test_bound_rejects_an_unwritten_last_column_of_the_second_channel_tile():
    x, w, b, gy, r, S = _fwd(_geo('C68 K65'))
    o = _f32(r)
    o[..., 64] = 0                                                   # `k < K - 1` in the store: column 64 keeps its old content
    assert _worst(o, r, S, FA.GAMMA_F32_CONV) > 1.0


def test_bound_rejects_a_tail_pixel_tile_written_from_row_zero():
    x, w, b, gy, r, S = _fwd(_geo('M129'))
    K = r.shape[-1]
    good = _f32(r).reshape(-1, K)
    o = good.clone()
    o[:1] = good[128:]                                               # the tail tile (row 128) stored at m - m0
    o[128:] = 0
    assert _worst(o.view(r.shape), r, S, FA.GAMMA_F32_CONV) > 1.0


def test_bound_rejects_a_dropped_last_split_and_splits_summed_twice():
    geo = ('wgrad', 1, 32, 1, 513, 32, 1, 1, 1, 0, 1)
    x, w, b, gy = _operands(geo)
    dw, S = FA.wgrad_ref(x, gy, 1, 1, 1, 0, 1)
    splits, per = FA.wgrad_plan(1, 1, 513, 32, 32, 1, 1)
    assert (splits, per) == (2, 264) and per % 64                   # a partial last 64-pixel chain as well
    assert _worst(_f32(dw), dw, S, FA.GAMMA_F32_WGRAD) <= 1.0
    parts = [FA.wgrad_ref(x[..., k * per:(k + 1) * per], gy[..., k * per:(k + 1) * per], 1, 1, 1, 0, 1)[0]
             for k in range(splits)]
    assert _worst(_f32(sum(parts)), dw, S, FA.GAMMA_F32_WGRAD) <= 1.0
    assert _worst(_f32(parts[0]), dw, S, FA.GAMMA_F32_WGRAD) > 1.0                          # the last split's pixels dropped
    assert _worst(_f32(sum(parts) + parts[1]), dw, S, FA.GAMMA_F32_WGRAD) > 1.0             # ... summed twice
    assert _worst(_f32(2 * sum(parts)), dw, S, FA.GAMMA_F32_WGRAD) > 1.0                    # every split summed twice
    # one pixel dropped: the last of the tail group of 8 (`p < p1 - 1`)
    one = FA.wgrad_ref(x[..., :-1], gy[..., :-1], 1, 1, 1, 0, 1)[0]
    assert _worst(_f32(one), dw, S, FA.GAMMA_F32_WGRAD) > 1.0


def test_bound_rejects_bias_added_to_the_data_gradient():
    geo = _geo('M128')                                               # K == C: a [K] bias fits dx's channels
    _, N, C, H, W, K, R, S_, stride, pad, dil = geo
    x, w, b, gy = _operands(geo)
    dx, S = FA.dgrad_ref(gy, w, H, W, stride, pad, dil)
    assert _worst(_f32(dx), dx, S, FA.GAMMA_F32_CONV) <= 1.0
    assert _worst(_f32(dx + b.double()), dx, S, FA.GAMMA_F32_CONV) > 1.0


def test_bound_rejects_a_nonzero_padded_channel_of_the_weight_gradient():
    geo = _geo('C3 K3')
    _, N, C, H, W, K, R, S_, stride, pad, dil = geo
    x, w, b, gy = _operands(geo)
    x4, g4 = F.pad(x, (0, 0, 0, 0, 0, 1)), F.pad(gy, (0, 0, 0, 0, 0, 1))       # what hip_conv_f32._nhwc hands the kernel
    dw, S = FA.wgrad_ref(x4, g4, R, S_, stride, pad, dil)
    assert bool((S[3] == 0).all()) and bool((S[:, 3] == 0).all()) and bool((S[:3, :3] > 0).all())
    o = _f32(dw)
    assert _worst(o, dw, S, FA.GAMMA_F32_WGRAD) <= 1.0
    o[1, 3, 0, 0] = 1e-12
    assert _worst(o, dw, S, FA.GAMMA_F32_WGRAD) > 1.0


def _emulated(signed, rows=2048, L=18432, seed=0):
    rs = np.random.RandomState(seed)
    a, w = rs.standard_normal((rows, L)).astype(np.float32), rs.standard_normal((rows, L)).astype(np.float32)
    if not signed:
        a, w = np.abs(a), np.abs(w)
    return a.astype(np.float64) * w.astype(np.float64)


def test_one_long_float32_chain_fails_where_the_blocked_sums_pass():
    """the numerical plant: correct code, another rounding order.  18432 same-signed products (2048 channels x 3 x 3, the
    DC5 reduction) summed in float32 as conv_f32_kernel does (chains of 32) and as the weight gradient does (chains of 64),
    and as one long chain: the blocked sums must pass the constants, the long chain must fail them."""
    prod = _emulated(signed=False)
    long_ = FA.sum_units(FA.chain_sum_f32(prod), prod)
    for block, gamma, name in ((32, FA.GAMMA_F32_CONV, 'conv'), (64, FA.GAMMA_F32_WGRAD, 'wgrad')):
        blocked = FA.sum_units(FA.blocked_sum_f32(prod, block), prod)
        print('%s: blocked (chains of %d) worst %.1f, one long chain worst %.1f, constant %.1f (units of 2^-24 S)' % (
            name, block, blocked.max(), long_.max(), gamma / FA.U))
        assert blocked.max() * FA.U <= gamma
        assert long_.max() * FA.U > gamma
    # signed products: reported, not asserted - see the comment above the constants
    prod = _emulated(signed=True)
    print('signed: blocked(32) worst %.2f, blocked(64) worst %.2f, one long chain worst %.2f' % (
        FA.sum_units(FA.blocked_sum_f32(prod, 32), prod).max(), FA.sum_units(FA.blocked_sum_f32(prod, 64), prod).max(),
        FA.sum_units(FA.chain_sum_f32(prod), prod).max()))


def test_constants_are_powers_of_two_twice_the_measurement_below_the_a_priori_bound():
    for g in (FA.GAMMA_F32_CONV, FA.GAMMA_F32_WGRAD):
        assert math.log2(g) == int(math.log2(g))
    # the longest audited reductions: 2048 x 3 x 3 (DC5's RPN convolution); the bench step's 512 splits of 2048 pixels
    assert FA.GAMMA_F32_CONV <= FA.conv_tree_bound(3, 3, 2048)
    assert FA.GAMMA_F32_WGRAD <= FA.wgrad_tree_bound(2048, 512)
    # the smallest power of two that is at least twice the measured worst
    for g, (worst, _) in ((FA.GAMMA_F32_CONV, FA.MEASURED['conv']), (FA.GAMMA_F32_WGRAD, FA.MEASURED['wgrad'])):
        assert 2.0 <= g / (worst * FA.U) < 4.0, g / (worst * FA.U)


# ------------------------------------------------------------------------------------------------- GPU audited fp32 steps
# what the RoI / loss half of an fp32 step launches (head_audit.Auditor's instantiations): fp32 maps take
# roi_align_fwd_rows_kernel<float> and the atomic backward; the RPN loss of an fp32 step takes the per-level CE + JSD
# launches (sigmoid rows: sig_kernel) in every config - the fused oadg_rpn_loss_fwd / _bwd reads the bf16 path's head map
# and is not launched here -; nothing is cast or permuted
_HEAD = {'cls_fin_kernel', 'parse_losses_kernel', 'roi_align_bwd_kernel', 'roi_align_fwd_rows_kernel<float>',
         'roi_order_rank_kernel', 'roi_reg_acc_fwd_kernel', 'roi_reg_bwd_kernel', 'sgd_multi_kernel', 'sig_kernel<false>',
         'sig_kernel<true>', 'sm_kernel<false>', 'sm_kernel<true>', 'supcon_bwd_fin_kernel', 'supcon_fin_kernel',
         'supcon_prep_kernel', 'supcon_tile_kernel<false>', 'supcon_tile_kernel<true>'}
HEAD_EXPECTED = {'r50_fpn_f32': _HEAD, 'r50_fpn_multiscale_f32': _HEAD, 'r101_dc5_f32': _HEAD}
HEAD_WRAPPERS = {'_RoIAlignFPN.forward', '_RoIAlignFPN.backward', '_CeJsd.forward', '_CeJsd.backward', '_RoiRegAcc.forward',
                 '_RoiRegAcc.backward', '_SupCon.forward', '_SupCon.backward', '_ParseLosses.forward', 'FusedSGD.step'}
HEAD_WRAPPERS_OF = {'r50_fpn_f32': HEAD_WRAPPERS, 'r50_fpn_multiscale_f32': HEAD_WRAPPERS, 'r101_dc5_f32': HEAD_WRAPPERS}
# the wrapper of head_audit.Auditor that verifies each launch label it claims
HEAD_VERIFIED_BY = {
    'oadg_roi_align_fwd': '_RoIAlignFPN.forward', 'oadg_roi_align_bwd': '_RoIAlignFPN.backward',
    'oadg_roi_align_bwd_tiles': '_RoIAlignFPN.backward', 'oadg_roi_order': '_RoIAlignFPN.backward',
    'oadg_roi_order_keys': '_RoIAlignFPN.backward', 'oadg_rpn_loss_fwd': '_RpnLoss.forward',
    'oadg_rpn_loss_bwd': '_RpnLoss.backward', 'oadg_ce_jsd_fwd': '_CeJsd.forward', 'oadg_ce_jsd_bwd': '_CeJsd.backward',
    'oadg_roi_reg_acc_fwd': '_RoiRegAcc.forward', 'oadg_roi_reg_bwd': '_RoiRegAcc.backward',
    'oadg_supcon_fwd': '_SupCon.forward', 'oadg_supcon_bwd': '_SupCon.backward', 'oadg_parse_losses': '_ParseLosses.forward',
    'oadg_fc_weight_permute': '_FcWeightPermute.forward', 'oadg_sgd_step_multi': 'FusedSGD.step',
}
F32_WRAPPERS = {'conv2d_f32', '_conv', '_conv transposed', '_wgrad', '_Conv2dF32.forward', '_Conv2dF32.backward'}
# the launch labels of conv_f32_kernel / the weight gradient in each audited step (f32_audit.conv_label / wgrad_label)
_CONV = {'conv_f32_kernel forward 1x1 s1 d1', 'conv_f32_kernel forward 1x1 s2 d1', 'conv_f32_kernel forward 3x3 s1 d1',
         'conv_f32_kernel forward 7x7 s2 d1 C4',                       # (the stem: C 3 -> 4, forward only)
         'conv_f32_kernel transposed 1x1 s1 d1', 'conv_f32_kernel transposed 1x1 s2 d1', 'conv_f32_kernel transposed 3x3 s1 d1',
         'conv_wgrad_f32_kernel + reduce 1x1 s1 d1, splits', 'conv_wgrad_f32_kernel + reduce 1x1 s2 d1, splits',
         'conv_wgrad_f32_kernel + reduce 3x3 s1 d1, splits'}
_R50 = _CONV | {'conv_f32_kernel forward 1x1 s1 d1 K3', 'conv_f32_kernel forward 1x1 s1 d1 K12',      # rpn_cls / rpn_reg
                'conv_f32_kernel transposed 1x1 s1 d1 C4', 'conv_f32_kernel transposed 1x1 s1 d1 C12',
                'conv_f32_kernel forward 3x3 s2 d1', 'conv_f32_kernel transposed 3x3 s2 d1',
                'conv_wgrad_f32_kernel + reduce 3x3 s2 d1, splits',
                'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K4, splits', 'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K12, splits'}
EXPECTED = {
    'r50_fpn_f32': _R50 | {'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K4, 512 splits',
                           'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K12, 512 splits'},
    # (the finest level's P = 4 x 200 x 400 = 320000: 512 splits of 632 pixels, and 507 x 632 > P - five empty splits)
    'r50_fpn_multiscale_f32': _R50 | {'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K4, 512 splits (empty trailing)',
                                      'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K12, 512 splits (empty trailing)'},
    # (dilated layer4, 15 / 60-channel heads padded to 16 / 60, the 2048 -> 2048 RPN convolution's one-split gradient)
    'r101_dc5_f32': _CONV | {'conv_f32_kernel forward 1x1 s1 d1 K15', 'conv_f32_kernel forward 1x1 s1 d1 K60',
                             'conv_f32_kernel transposed 1x1 s1 d1 C16', 'conv_f32_kernel transposed 1x1 s1 d1 C60',
                             'conv_f32_kernel forward 3x3 s1 d2', 'conv_f32_kernel transposed 3x3 s1 d2',
                             'conv_wgrad_f32_kernel + reduce 3x3 s1 d2, splits',
                             'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K16, splits',
                             'conv_wgrad_f32_kernel + reduce 1x1 s1 d1 K60, splits',
                             'conv_wgrad_f32_kernel + reduce 3x3 s1 d1, 1 split'},
}


def _f32_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size, key, fused_anchor_targets=True):
    A, H_, T = FA.Auditor(), HA.Auditor(), TA.Auditor()
    library, checked = [], []

    def install(mp, det):
        A.install(mp, det)
        H_.install(mp, det)
        T.install(mp, det)
        conv2d = F.conv2d
        mp.setattr(F, 'conv2d', lambda *a, **k: (library.append(tuple(a[1].shape)), conv2d(*a, **k))[1])

    def on_begin():
        A.params.clear()                                 # (a step repeated on the host sampler's path starts over)

    def on_end_backward(det):
        checked.append(A.check_params(list(det.named_parameters())))

    out, det, wall = audited_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size, install, on_begin,
                                  on_end_backward, before_step1=lambda mp, det: H_.install_sgd(mp, det), amp_dtype=None)
    drew_on_device = T.check_end_state()
    title = '%s (audited fp32 step %.1f s)' % (key, wall)
    A.print_table(title)
    H_.print_table(title)
    T.print_table(title)
    print('worst err / bound: f32 convolutions %.4f, heads / losses / SGD %.4f, targets %.4f' % (A.worst(), H_.worst(),
                                                                                                  T.worst()))
    print('f32 launch labels:', sorted(A.kernels))
    print('head instantiations:', sorted(H_.kernels))
    print('library convolutions:', library)
    seen = set(T.labels) | set(A.labels) | ({'oadg_host_randperm_prefix', 'oadg_np_random_bboxes'} & T.checked)
    head = {LABEL_OF.get(s, s) for s in HA.CLAIMS}
    print('labels seen:', sorted(seen))
    print('parameters checked: %d' % len(checked[-1] if checked else ()))
    print('labels no auditor verified:', sorted(seen - FA.CLAIMS - head - T.checked),
          sorted(s for s in seen & head if HEAD_VERIFIED_BY[s] not in H_.wrappers))
    trainable = {n for n, p in det.named_parameters() if p.requires_grad and n.startswith(('backbone.', 'neck.', 'rpn_head.'))}
    print('trainable convolution parameters without a gradient check:', sorted(trainable - (checked[-1] if checked else set())))
    assert not A.failures, A.failures[:10]
    assert not H_.failures, H_.failures[:10]
    assert not T.failures, T.failures[:10]
    for aud, want in ((A, F32_WRAPPERS), (H_, HEAD_WRAPPERS_OF[key]), (T, TARGET_WRAPPERS)):
        assert not want - set(aud.wrappers), want - set(aud.wrappers)
    assert A.kernels == EXPECTED[key], (sorted(A.kernels - EXPECTED[key]), sorted(EXPECTED[key] - A.kernels))
    assert H_.kernels == HEAD_EXPECTED[key], (sorted(H_.kernels - HEAD_EXPECTED[key]), sorted(HEAD_EXPECTED[key] - H_.kernels))
    # no library convolution anywhere in the detector's step, and nothing declined by the dispatcher
    assert not library and A.declined == 0, (library, A.declined)
    # closure at run time: every label a check() saw during the audited step belongs to one of the three auditors and was
    # verified by it
    unclaimed = seen - FA.CLAIMS - head - T.checked
    assert not unclaimed, sorted(unclaimed)
    assert seen & FA.CLAIMS == A.checked == FA.CLAIMS, (sorted(seen & FA.CLAIMS), sorted(A.checked))
    unverified = {s for s in seen & head if HEAD_VERIFIED_BY[s] not in H_.wrappers}
    assert not unverified, sorted(unverified)
    want = CHECKED['device'] - (set() if fused_anchor_targets else {'oadg_anchor_targets'})
    assert T.checked == want, (sorted(T.checked - want), sorted(want - T.checked))
    # every trainable convolution parameter's gradient went through the parameter pass
    assert trainable and checked and checked[-1] == trainable, sorted(trainable ^ checked[-1])[:10]
    assert [s[0::2] for s in H_.info['sgd_steps']] == [('first step', 'fused'), ('later step', 'fused')], H_.info['sgd_steps']
    assert not H_.info['sgd_missed'], H_.info['sgd_missed'][:10]
    for fam, (carved, total) in H_.borderline.items():
        assert carved <= BORDERLINE_CAP * max(total, 1), (fam, carved, total)
    # positives exist in both samplers, proposals were kept, the device sampler drew (the conditions of the bf16 target audit)
    assert drew_on_device and not T.declined, T.declined
    assert T.n_pos['rpn'] and min(T.n_pos['rpn']) > 0 and T.n_pos['roi'] and min(T.n_pos['roi']) > 0, T.n_pos
    roi = [d for d in T.draws if d['kind'] == 'roi']
    assert len(roi) == batch and all(d['branch'] == 'device' and d['k_pos'] > 0 and d['k_pos'] + d['k_neg'] == 512 for d in roi)
    assert T.info['proposals'] == 'fused' and all(k > 0 for k in T.info['proposals_kept'])
    assert T.info['anchor_targets'] == ('fused' if fused_anchor_targets else 'tensor path')
    assert T.one_sided == 0 and not T.borderline, (T.one_sided, T.borderline)
    return A, H_, T


@pytest.mark.gpu
def test_f32_audit_config1_r50_fpn_bench_step(dev, monkeypatch):
    """configs[1] as ``bench.py --dtype fp32`` builds it: 4 images x 2 views at 1024 x 2048 - M = 4.2 M pixels at the stem,
    512-split weight gradients of the 3 / 12-channel heads, the stem's C 3 -> 4"""
    _f32_step(dev, monkeypatch, R50_CFG, 4, 1024, 2048, 20, 8, (24, 400), 'r50_fpn_f32')


@pytest.mark.gpu
def test_f32_audit_multiscale_800x1600(dev, monkeypatch):
    """2 images x 2 views at 800 x 1600: ragged M (80000 / 20000 / 5000 / 1300 per level), partial pixel tiles, partial
    8-pixel groups, empty trailing splits"""
    _f32_step(dev, monkeypatch, R50_CFG, 2, 800, 1600, 12, 8, (24, 300), 'r50_fpn_multiscale_f32')


@pytest.mark.gpu
def test_f32_audit_config3_r101_dc5(dev, monkeypatch):
    """R101-DC5 at 736 x 1280: dilation 2 / pad 2, 18432-product reductions, K = 15 / 60 heads, one-split weight gradients"""
    _f32_step(dev, monkeypatch, DC5_CFG, 2, 736, 1280, 12, 7, (24, 300), 'r101_dc5_f32', fused_anchor_targets=False)


# ----------------------------------------------------------------------------------------------- GPU stress launches
def _launch(dev, geo, relu=False, positive=False, bias=True, need=(True, True, True), seed=0):
    """conv2d_f32 forward + backward on the device (under whatever auditor is installed); returns (y, dx, dw, db)"""
    from oadg_amd import hip_conv_f32
    _, N, C, H, W, K, R, S, stride, pad, dil = geo
    x, w, b, gy = _operands(geo, seed=seed, relu=relu, positive=positive, bias=bias, device=dev)
    x.requires_grad_(need[0])
    w.requires_grad_(need[1])
    if b is not None:
        b.requires_grad_(need[2])
    y = hip_conv_f32.conv2d_f32(x, w, b, stride, pad, dil)
    assert y is not None and tuple(y.shape) == tuple(gy.shape)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


def _finish(A, title, monkeypatch):
    torch.cuda.synchronize()
    monkeypatch.undo()
    A.print_table(title)
    assert not A.failures, A.failures[:10]
    assert A.checked <= FA.CLAIMS and set(A.labels) <= FA.CLAIMS
    return A


@pytest.mark.gpu
@pytest.mark.parametrize('inputs', ['signed', 'post-ReLU'])
def test_f32_stress_geometries(dev, monkeypatch, inputs):
    """every geometry of the list, forward + dx + dW + db, with and without bias (alternating)"""
    A = FA.Auditor().install(monkeypatch)
    for i, geo in enumerate(GEOMETRIES):
        y, dx, dw, db = _launch(dev, geo, relu=inputs == 'post-ReLU', bias=i % 2 == 0)
        assert dx is not None and dw is not None and (db is not None) == (i % 2 == 0)
    _finish(A, 'stress geometries, %s inputs' % inputs, monkeypatch)
    calls = len(GEOMETRIES)
    assert A.wrappers == {'conv2d_f32': calls, '_conv': calls, '_conv transposed': calls, '_wgrad': calls,
                          '_Conv2dF32.forward': calls, '_Conv2dF32.backward': calls}, A.wrappers
    assert A.checked == FA.CLAIMS
    zero = [k for k in A.table if k.endswith('exactly zero where nothing is summed (some)')]
    assert any('transposed 1x1 s2' in k for k in zero) and any('C4' in k for k in zero), zero


@pytest.mark.gpu
def test_f32_stress_same_signed_long_reductions(dev, monkeypatch):
    """non-negative inputs, weights and output gradients on the DC5 reduction (2048 channels x 3 x 3 = 18432 products,
    dilation 2; the weight gradient's 9216 pixels in one split): every product of a chain has the same sign - the worst
    case of a summation order, which the steps' signed weights do not reach"""
    A = FA.Auditor().install(monkeypatch)
    assert FA.wgrad_plan(2, 48, 96, 2048, 2048, 3, 3) == (1, 9216)
    _launch(dev, ('same-signed DC5', 2, 2048, 48, 96, 2048, 3, 3, 1, 2, 2), positive=True)
    _finish(A, 'same-signed 18432-product reductions', monkeypatch)
    assert A.longest['conv'] == 18432 and A.longest['wgrad'] == (9216, 1)


@pytest.mark.gpu
def test_f32_stress_weight_gradient_splits(dev, monkeypatch):
    """P = 511, 512, 513 (one / two splits, a partial last 64-pixel chain), a (K, C, P) whose trailing splits are empty,
    the 1024-split cap"""
    A = FA.Auditor().install(monkeypatch)
    cases = [(1, 7, 73, 32, 32), (1, 16, 32, 32, 32), (1, 19, 27, 32, 32), (1, 481, 545, 256, 3), (1, 1, 524389, 32, 3)]
    plans = [FA.wgrad_plan(N, H, W, C, (K + 3) // 4 * 4, 1, 1) for N, H, W, C, K in cases]
    assert plans[:3] == [(1, 512), (1, 512), (2, 264)] and 264 % 64
    # trailing splits that start behind P: per_split is rounded up to a multiple of 8
    assert plans[3] == (512, 520) and FA.empty_trailing_splits(481 * 545, 512, 520) == 7 and 505 * 520 >= 481 * 545
    assert plans[4][0] == 1024
    for N, H, W, C, K in cases:
        _launch(dev, ('wgrad', N, C, H, W, K, 1, 1, 1, 0, 1), relu=True, need=(False, True, True))
    _finish(A, 'weight-gradient splits', monkeypatch)
    assert A.wrappers['_wgrad'] == len(cases) and '_conv transposed' not in A.wrappers
    assert any('512 splits (empty trailing)' in k for k in A.kernels) and any('1024 splits' in k for k in A.kernels), A.kernels


@pytest.mark.gpu
def test_f32_stress_needs_input_grad_and_the_declined_call(dev, monkeypatch):
    """frozen weights: only dx; the first layer: only dW; no bias gradient without a bias.  Padding (0, 1) is outside the
    kernels' domain: conv2d_f32 returns None, nothing launches, and layers.conv2d falls back to the library"""
    from oadg_amd import hip_conv_f32, layers
    A = FA.Auditor().install(monkeypatch)
    geo = _geo('C36 K64')
    y, dx, dw, db = _launch(dev, geo, need=(True, False, False))
    assert dx is not None and dw is None and db is None and A.wrappers.get('_wgrad') is None
    y, dx, dw, db = _launch(dev, geo, need=(False, True, True))
    assert dx is None and dw is not None and db is not None and A.wrappers['_conv transposed'] == 1
    y, dx, dw, db = _launch(dev, geo, bias=False, need=(False, True, True))
    assert dw is not None and db is None
    x, w, b, gy = _operands(_geo('1x3'), device=dev)
    assert hip_conv_f32.conv2d_f32(x, w, None, 1, (0, 1), 1) is None and A.declined == 1
    library = []
    conv2d = F.conv2d
    monkeypatch.setattr(F, 'conv2d', lambda *a, **k: (library.append(1), conv2d(*a, **k))[1])
    y = layers.conv2d(x, w, None, 1, (0, 1), 1)
    assert len(library) == 1 and A.declined == 2
    ref = conv2d(x.double().cpu(), w.double().cpu(), None, 1, (0, 1), 1)
    S = conv2d(x.double().cpu().abs(), w.double().cpu().abs(), None, 1, (0, 1), 1)
    assert tuple(y.shape) == tuple(ref.shape) and bool(((y.double().cpu() - ref).abs() <= FA.conv_tree_bound(1, 3, 8) * S).all())
    _finish(A, 'needs_input_grad combinations, declined call', monkeypatch)


@pytest.mark.gpu
def test_f32_launches_are_bit_identical_from_run_to_run(dev, monkeypatch):
    """fixed split order, no atomics: once per family, two runs of the same launch give the same bits"""
    A = FA.Auditor().install(monkeypatch)
    for geo in (_geo('M65884'), ('wgrad 512 splits', 1, 256, 481, 545, 3, 1, 1, 1, 0, 1)):
        a = _launch(dev, geo)
        b = _launch(dev, geo)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    _finish(A, 'bit-identical reruns', monkeypatch)
