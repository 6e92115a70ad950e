"""Stress suite of RoIAlign (csrc/roi_align.hip) on the cases of tests/roi_cases.py: pooled shapes other than 7 x 7, fixed
sampling ratios, unaligned RoIs, the weight tables' overflow thresholds (FR_SPAN 32, RB_SPAN 96), channel counts that are no
multiple of 64, tiny and ragged maps, 2 .. 8 tiles per workgroup with a ragged last one, bad batch indices and degenerate
boxes, more than 8192 RoIs (the host-side sort) and none.

GPU tests (-m gpu) drive hip_ops.roi_align_fpn forward and backward under head_audit.Auditor: every launch is checked
element by element against fp64 from the operands it received, with head_audit's bound unchanged; each test asserts the set
of kernels launched and that no borderline RoI took the other side of its choice (``roi_other_side == 0``).  fp32 maps take
the rows forward and the atomic backward, bf16 maps the rows forward and the tile backward.

CPU self-tests (no mark): the fp64 references equal oracle/roi_align.py at the parameter combinations the GPU tests use, the
checker rejects planted errors, and every case reaches the path it is named for (roi_cases.Case.check).
"""
import pytest
import torch

import head_audit as HA
import roi_cases as R
from oracle import roi_align as ORA

gpu = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ORACLE_BAR = 0.25            # tests/test_head_audit.py's bar for an fp32 oracle against the fp64 reference


def _worst(o, ref, b):
    return HA.ratio(o, ref, b)[0]


def _cpu_feats(case, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(s, generator=g) for s in case.shapes]


def _ref_fwd(case, feats, geo=None, lvl=None, rho=0.0):
    r, S, S4 = HA.roi_align_ref(feats, case.rois, case.lvl if lvl is None else lvl, case.geo if geo is None else geo,
                                case.PH, case.PW)
    return r, HA.bound(r, S, rho, HA.GAMMA_ROI, HA.POS_ERR * S4)


def _ref_bwd(case, gout, rho=0.0):
    refs = HA.roi_align_bwd_ref(case.shapes, case.rois, case.lvl, case.geo, gout, case.PH, case.PW)
    return [(r, HA.bound(r, S, rho, HA.GAMMA_ROI, HA.POS_ERR * S4)) for r, S, S4 in refs]


def _oracle(case, feats, rois=None):
    return ORA.roi_align_fpn(feats, case.rois if rois is None else rois, (case.PH, case.PW), [1 / s for s in case.scales],
                             case.finest, case.sr, case.aligned)


# ====================================================================================================== CPU self-tests
ORACLE_COMBOS = [(7, 7, 2, True), (7, 7, 0, False), (7, 7, 2, False), (8, 8, 0, True), (5, 7, 0, True), (7, 5, 2, False),
                 (14, 14, 0, True), (14, 14, 2, True), (1, 1, 0, True), (3, 8, 0, True)]


def _oracle_case(PH, PW, sr, aligned):
    if (PH, PW, sr, aligned) == ('wide', 0, 0, True):
        # a 112-pixel bin on a 16 x 800 map
        return R.Case('oracle/wide', ((16, 800),), torch.tensor([[0, 8.8, 3.4, 8.8 + 7 * 111.7, 3.4 + 7 * 1.3]]), N=1,
                      scales=(1.0,))
    if PH == 'threshold':
        c = R.threshold_case('x')
        k = R.THRESHOLD_BINS.index(97)
        return R.Case('oracle/threshold 97', R.WIDE_X, c.rois[k:k + 1], scales=(1.0,))
    rois = torch.cat([R.rand_rois(40, 1), R.tiny_rois(8, 2)])
    return R.settle(R.Case('oracle/%dx%d sr%d %s' % (PH, PW, sr, aligned), R.PYRAMID, rois, PH=PH, PW=PW, sr=sr, aligned=aligned))


@pytest.mark.parametrize('combo', ORACLE_COMBOS + [('wide', 0, 0, True), ('threshold', 0, 0, True)], ids=str)
def test_references_match_the_oracle(combo):
    """forward and backward fp64 references against oracle/roi_align.py (fp32 arithmetic of the published kernel)"""
    case = _oracle_case(*combo)
    feats = _cpu_feats(case)
    r, b = _ref_fwd(case, feats)
    assert bool((r != 0).any())
    assert _worst(_oracle(case, feats).permute(0, 2, 3, 1).double(), r, b) <= ORACLE_BAR
    gout = case.gout(F32, 'cpu')
    fs = [f.clone().requires_grad_(True) for f in feats]
    _oracle(case, fs).backward(gout)
    for f, (r, b) in zip(fs, _ref_bwd(case, gout)):
        o = (f.grad if f.grad is not None else torch.zeros_like(f)).permute(0, 2, 3, 1).double()
        assert _worst(o, r, b) <= ORACLE_BAR
        assert torch.equal(o == 0, r == 0)


def test_rejects_an_unaligned_roi_without_the_one_pixel_minimum():
    case = R.sampling_case(2, False)
    feats = _cpu_feats(case)
    r, b = _ref_fwd(case, feats)
    assert _worst(_oracle(case, feats).permute(0, 2, 3, 1).double(), r, b) <= ORACLE_BAR
    raw = case.rois.double()
    sc = torch.tensor(case.scales, dtype=torch.float64)[case.lvl]
    geo = dict(case.geo, bw=(raw[:, 3] - raw[:, 1]) * sc / case.PW, bh=(raw[:, 4] - raw[:, 2]) * sc / case.PH)
    bad, _ = _ref_fwd(case, feats, geo=geo)
    tiny = (geo['bw'] * case.PW < 1) | (geo['bh'] * case.PH < 1)
    assert int(tiny.sum()) >= 16 and not bool(tiny.all())
    for k in tiny.nonzero().view(-1).tolist():
        assert _worst(bad[k], r[k], b[k]) > 1.0
    assert _worst(bad[~tiny], r[~tiny], b[~tiny]) <= 1.0          # (RoIs of a pixel or more: the rule changes nothing)


def test_rejects_adaptive_counts_where_the_sampling_ratio_is_two():
    case, adaptive = R.sampling_case(2, True), R.Case('adaptive', R.PYRAMID, R.sampling_case(2, True).rois, sr=0)
    feats = _cpu_feats(case)
    r, b = _ref_fwd(case, feats)
    bad, _ = _ref_fwd(adaptive, feats)
    assert _worst(bad, r, b) > 1.0


def test_rejects_swapped_pooled_sides():
    case, swapped = R.pooled_case(5, 7), R.Case('swapped', R.PYRAMID, R.pooled_case(5, 7).rois, PH=7, PW=5)
    feats = _cpu_feats(case)
    r, b = _ref_fwd(case, feats)
    bad, _ = _ref_fwd(swapped, feats)                              # [K, 7, 5, C] read as [K, 5, 7, C]
    assert _worst(bad.reshape(r.shape), r, b) > 1.0
    assert _worst(bad.permute(0, 2, 1, 3), r, b) > 1.0


def test_rejects_a_backward_without_the_bins_past_the_fourth_on_a_tile():
    case = R.subpixel_case().check()
    gout = case.gout(F32, 'cpu')
    (r, b), _, _ = _ref_bwd(case, gout, rho=HA.RHO)
    assert _worst(HA.bf16(r), r, b) <= 1.0
    rows, cols = gout.clone(), gout.clone()
    rows[:, :, 4:, :] = 0                                          # bin rows 4 .. 7 of every RoI dropped
    cols[:, :, :, 4:] = 0
    for g2 in (rows, cols):
        bad = HA.roi_align_bwd_ref(case.shapes, case.rois, case.lvl, case.geo, g2, 8, 8)[0][0]
        assert _worst(HA.bf16(bad), r, b) > 1.0


def test_rejects_an_unwritten_last_tile_of_an_image():
    case = R.tpw_case('tpw5').check()
    gout = case.gout(F32, 'cpu')
    (r, b), = _ref_bwd(case, gout, rho=HA.RHO)
    o = HA.bf16(r)
    assert _worst(o, r, b) <= 1.0
    H = case.shapes[0][2]
    for n in range(case.N):                                        # the one-tile last workgroup of image n never flushed
        bad = o.clone()
        bad[n, H - 8:, H - 8:] = 0
        assert _worst(bad, r, b) > 1.0


def test_reference_gives_zeros_for_bad_batch_indices_and_degenerate_boxes():
    case = R.degenerate_case().check()
    feats = _cpu_feats(case)
    r, b = _ref_fwd(case, feats)
    assert not bool(r[case.degenerate].any()) and bool((r[~case.degenerate] != 0).any())
    assert _worst(_oracle(case, feats).permute(0, 2, 3, 1).double(), r, b) <= ORACLE_BAR
    gout = case.gout(F32, 'cpu')
    g2 = gout.clone()
    g2[case.degenerate] = 0
    for (r1, _), (r2, _) in zip(_ref_bwd(case, gout), _ref_bwd(case, g2)):
        assert torch.equal(r1, r2)                                 # they contribute nothing backward


def test_order_check_follows_the_kernel_on_nan_and_inverted_boxes():
    """roi_order_key clamps the extents with fmaxf (NaN -> 0) and converts a NaN cell to 0: the reference keys must be defined
    there too - a stable sort of them passes, a swap of two distinct keys does not"""
    case = R.degenerate_case()
    keys, grp = HA.roi_order_expect(case.rois, case.N, 3, case.finest)[0]
    assert int(keys.min()) >= 0 and int(grp.max()) < 3 * case.N
    nan = torch.isnan(case.rois).any(1)
    assert bool(nan.any()) and bool((grp[nan] // case.N == 0).all())           # extent 0: level 0
    order = torch.sort(keys, stable=True)[1].int()
    rng = torch.searchsorted(grp[order.long()], torch.arange(3 * case.N + 1)).int()
    assert HA.check_order(case.rois, case.N, 3, case.finest, order, rng)[0]
    sk = keys[order.long()]
    i = int((sk[1:] != sk[:-1]).nonzero()[0])
    bad = order.clone()
    bad[i], bad[i + 1] = order[i + 1], order[i]
    assert not HA.check_order(case.rois, case.N, 3, case.finest, bad, rng)[0]


def test_order_check_rejects_an_unstable_sort_of_tied_keys():
    case = R.big_case(R.BIG_K[0])
    keys, grp = HA.roi_order_expect(case.rois, case.N, 3, case.finest)[0]
    order = torch.sort(keys, stable=True)[1].int()
    assert HA.check_order(case.rois, case.N, 3, case.finest, order, None)[0]
    sk = keys[order.long()]
    i = int((sk[1:] == sk[:-1]).nonzero()[0])
    bad = order.clone()
    bad[i], bad[i + 1] = order[i + 1], order[i]                    # two RoIs of one cell in the other order
    assert not HA.check_order(case.rois, case.N, 3, case.finest, bad, None)[0]


@pytest.mark.parametrize('case', R.all_cases(), ids=repr)
def test_case_reaches_its_path(case):
    assert case.claims
    case.check()


def test_thresholds_have_both_sides():
    for axis in 'xy':
        c = R.threshold_case(axis)
        span = c.spans[1 if axis == 'x' else 0]
        for T, mask in ((R.FR_SPAN, c.fwd_per_sample), (R.RB_SPAN, c.bwd_scatter)):
            assert {T - 1, T, T + 1} <= set(span.tolist())
            assert bool(mask[span == T].all()) and not bool(mask[span == T - 1].any())


def test_expected_kernel_sets():
    c = R.pooled_case(14, 14)
    assert c.kernels(BF16) == {R.FWD[BF16], 'roi_align_bwd_kernel'} and c.kernels(F32) == {R.FWD[F32], 'roi_align_bwd_kernel'}
    c = R.pooled_case(8, 8)
    assert c.kernels(BF16) == {R.FWD[BF16], 'roi_align_bwd_tiles_kernel', 'roi_tile_box_kernel', 'roi_order_rank_kernel'}
    c = R.big_case(R.BIG_K[0])
    assert c.kernels(F32) == {R.FWD[F32], 'roi_align_bwd_kernel', 'roi_order_key_kernel'}
    assert c.kernels(BF16) == {R.FWD[BF16], 'roi_align_bwd_tiles_kernel', 'roi_tile_box_kernel', 'roi_order_key_kernel'}


# =========================================================================================================== GPU tests
def _run(dev, monkeypatch, case, dt, audit=True):
    """one forward + backward of ``case`` under the auditor: (auditor, output, map gradients)"""
    from oadg_amd import hip_ops
    case.check()
    feats = case.feats(dt, dev)
    A = HA.Auditor().install(monkeypatch, sgd=False) if audit else None
    out = hip_ops.roi_align_fpn(feats, case.rois.to(dev), (case.PH, case.PW), list(case.scales), case.finest, case.sr,
                                case.aligned)
    out.backward(case.gout(dt, dev))
    torch.cuda.synchronize()
    grads = [f.grad for f in feats]
    if not audit:
        return None, out.detach(), grads
    monkeypatch.undo()
    A.print_table('%s %s' % (case.name, dt))
    print('worst err / bound: %s %s %.4f' % (case.name, dt, A.worst()))
    assert not A.failures, A.failures[:10]
    assert A.info.get('roi_other_side', 0) == 0, A.info
    assert A.wrappers == {'_RoIAlignFPN.forward': 1, '_RoIAlignFPN.backward': 1}, A.wrappers
    assert A.kernels == case.kernels(dt), (sorted(A.kernels), sorted(case.kernels(dt)))
    assert all(g is not None and g.dtype == dt and g.shape == f.shape for g, f in zip(grads, feats))
    return A, out.detach(), grads


def _both(case):
    return [pytest.param(case, dt, id='%s-%s' % (case.name, 'fp32' if dt == F32 else 'bf16')) for dt in case.dtypes]


def _params(cases):
    return [p for c in cases for p in _both(c)]


@gpu
@pytest.mark.parametrize('case,dt', _params([R.pooled_case(*p) for p in R.POOLED] + [R.subpixel_case()]))
def test_pooled_shapes(dev, monkeypatch, case, dt):
    """PW = 8: the per-sample form inside the rows kernel; PH = 8, PW <= 7: two bin rows per wave; a side above 8: forward per
    sample, backward per-sample scatter, bf16 off the tile kernel; 8 x 8 on sub-pixel RoIs: the tile kernel's further 4 x 4
    bin blocks"""
    _run(dev, monkeypatch, case, dt)


@gpu
@pytest.mark.parametrize('case,dt', _params([R.sampling_case(sr, al) for sr in (1, 2, 3) for al in (True, False)] +
                                            [R.sparse_case(k, a) for k in ('gaps', 'overflow') for a in 'xy']))
def test_sampling_parameters(dev, monkeypatch, case, dt):
    """fixed sample counts, the unaligned max(rw, 1) rule on RoIs below one pixel (the tile rectangle follows it), two-sample
    bins with zero-weight rows between the samples and two-sample bins that overflow FR_SPAN"""
    _run(dev, monkeypatch, case, dt)


@gpu
@pytest.mark.parametrize('case,dt', _params([R.threshold_case(a) for a in ('x', 'y', 'xy')]))
def test_table_thresholds(dev, monkeypatch, case, dt):
    """bins of 31 / 32 / 33 and 95 / 96 / 97 pixels along one axis: both sides of the rows forward's and of the atomic
    backward's table overflow (roi_bwd_scatter with PH <= 8 from 96 pixels on); 33 x 33: both tables overflow"""
    _run(dev, monkeypatch, case, dt)


@gpu
@pytest.mark.parametrize('case,dt', _params([R.channel_case(C) for C in R.CHANNELS]))
def test_channel_counts(dev, monkeypatch, case, dt):
    """partial lanes, a partial 64-channel wave (chan_ok), a second chunk of 4 or 8 channels on blockIdx.y, the atomic
    backward's c < C guards"""
    _run(dev, monkeypatch, case, dt)


@gpu
@pytest.mark.parametrize('case,dt', _params([R.tiny_level_case(*s) for s in R.TINY_LEVELS] + [R.tiny_pyramid_case()]))
def test_tiny_and_ragged_maps(dev, monkeypatch, case, dt):
    """maps down to 1 x 1; RoIs that cover the map and hang over every side, lie wholly outside on each of the four sides, start
    in (-1, 0] and end between size - 1 and size"""
    _run(dev, monkeypatch, case, dt)


@gpu
@pytest.mark.parametrize('case,dt', _params([R.tpw_case(k) for k in ('tpw5', 'tpw2', 'tpw8')]))
def test_tiles_per_workgroup(dev, monkeypatch, case, dt):
    """5, 2 (two channel chunks) and 8 (a group of more than 512 RoIs) tiles per workgroup, each with a ragged last workgroup
    per image and RoIs on its tiles"""
    _run(dev, monkeypatch, case, dt)


@gpu
@pytest.mark.parametrize('case,dt', _both(R.degenerate_case()))
def test_bad_batch_indices_and_degenerate_boxes(dev, monkeypatch, case, dt):
    """batch -1 / N / N + 5, zero area, inverted on one and on both axes, a NaN coordinate: zero output, nothing backward"""
    A, out, grads = _run(dev, monkeypatch, case, dt)
    assert not bool(out[case.degenerate.to(dev)].any())
    assert bool(out[(~case.degenerate).to(dev)].any(dim=0).any())


@gpu
@pytest.mark.parametrize('case,dt', _params([R.big_case(K) for K in R.BIG_K]))
def test_more_than_8192_rois(dev, monkeypatch, case, dt):
    """the key kernel and the host-side sort: audited values, the order check (a stable sort of tied keys), and for bf16 a
    second run bit-identical to the first"""
    A, out, grads = _run(dev, monkeypatch, case, dt)
    assert A.table['roi_order_key_kernel order / range'].worst == 0.0
    if dt == BF16:
        _, out2, grads2 = _run(dev, monkeypatch, case, dt, audit=False)
        assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('size', [(7, 7), (14, 14)], ids=['7x7', '14x14'])
@pytest.mark.parametrize('entry', ['roi_align_fpn', 'RoIAlign layer'])
def test_no_rois(dev, entry, size, dt):
    """K = 0: an empty [0, C, PH, PW] output and zero gradients of the maps' shape and dtype.  (No auditor: there is no launch.
    Before this suite oadg_roi_align_fwd answered OADG_EARG to the NULL pointers of the empty tensors.)"""
    from oadg_amd import hip_ops, roi_heads
    g = torch.Generator().manual_seed(5)
    sizes = R.PYRAMID if entry == 'roi_align_fpn' else R.PYRAMID[:1]
    feats = [torch.randn((2, 8) + s, generator=g).to(dev, dt).requires_grad_(True) for s in sizes]
    rois = torch.zeros((0, 5), device=dev)
    if entry == 'roi_align_fpn':
        out = hip_ops.roi_align_fpn(feats, rois, size, [0.25, 0.125, 0.0625], 8, 0, True)
    else:
        out = roi_heads.RoIAlign(size, spatial_scale=0.25)(feats[0], rois)
    assert out.shape == (0, 8) + size and out.dtype == dt
    out.sum().backward()
    torch.cuda.synchronize()
    for f in feats:
        assert f.grad is not None and f.grad.shape == f.shape and f.grad.dtype == dt and not bool(f.grad.any())
