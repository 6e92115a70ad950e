"""Stress suite of the selection kernels: the two-kernel NMS (csrc/nms.hip) and the radix-select top-k, level merge, decode
and gather kernels (csrc/proposals.hip), on the constructed cases of tests/select_cases.py.  Their outputs are index lists:
every comparison is array_equal / torch.equal, there are no tolerances.

GPU tests (-m gpu) call the C ABI through _lib directly.  The NMS families run at 4,497 / 12,000 / 12,288 rows
(nms_scan_kernel<3, 2>) and at 12,289 / 16,385 / 32,768 rows (nms_scan_kernel<MAX_WORDS_PER_LANE, 1>, never launched by any
other module) against the O(M) Fraction reference; every NMS launch here gets a workspace and keep buffers pre-filled with
0xFF bytes.  Limits launched: 32,768 rows per image, 48 top-k rows, k = 16,384, eight levels, M = 19,199 merged candidates;
one past each limit must return OADG_EARG (and RPNHead.get_bboxes must take its sort path there).

CPU self-tests (no mark): the Fraction reference equals oracle.nms.nms_sorted on every family at 4,497 rows or fewer, and
every planted wrong scan / wrong top-k changes the list of the case named for it."""
import ctypes

import numpy as np
import pytest
import torch

import select_cases as S
from oracle import nms as ONMS

gpu = pytest.mark.gpu
OADG_EARG, OADG_ESIZE = -1, -2
ALL_SIZES = S.NARROW_SIZES + S.WIDE_SIZES
FAMILIES = tuple(f for f in S.NMS_FAMILIES if f != 'disjoint')
_SCANS_LAUNCHED = set()


# ====================================================================================================== CPU self-tests
def _small_cases(family):
    if family == 'disjoint':
        return [c for M in (1, 63, 64, 65) for c in S.nms_family('disjoint', M)]
    return S.counts_cases(4497)[2] if family == 'counts' else S.nms_family(family, 4497)


@pytest.mark.parametrize('family', S.NMS_FAMILIES + ('counts',))
def test_fraction_reference_equals_the_dense_oracle(family):
    """every family at <= 4,497 rows: the per-cell Fraction scan, the row-order scan and oracle.nms.nms_sorted (fp32 IoU
    matrix) give one list"""
    cases = _small_cases(family)
    assert cases and all(c.name.split('/')[0] == family for c in cases)
    for case in cases:
        ref = case.expected()
        boxes = case.boxes()[:case.count]
        dense = ONMS.nms_sorted(boxes, float(case.thr), case.max_keep) if case.count else np.zeros(0, np.int64)
        assert np.array_equal(ref, dense), case.name
        assert np.array_equal(ref, S.planted_scan(case)), case.name


@pytest.mark.parametrize('bug,where', [
    ('suppressed_suppress', ('chain', 0)), ('drop_far', ('far', 0)), ('drop_dist3', ('first_needed', 0)),
    ('first16_far', ('far', 0)), ('first8_far', ('far', 0)), ('ge', ('strict', 0)), ('past_counts', ('counts', 1))])
def test_planted_scan_changes_its_named_case(bug, where):
    family, i = where
    case = S.counts_cases(4497)[2][i] if family == 'counts' else S.nms_family(family, 4497)[i]
    if bug == 'ge':
        assert case.name.endswith('/at')
    if bug == 'past_counts':
        assert case.count == 1
    ref, got = case.expected(), S.planted_scan(case, bug)
    assert not np.array_equal(ref, got), (bug, case.name)
    if bug == 'suppressed_suppress':           # the chain's last row is what goes missing
        assert set(ref) - set(got) == {ch['c'] for ch in case.chains}


def test_planted_scans_are_rejected_at_every_size():
    """at every size a GPU test runs, the family named for a planted error rejects it"""
    named = {'suppressed_suppress': 'chain', 'drop_far': 'far', 'drop_dist3': 'first_needed', 'first16_far': 'far',
             'first8_far': 'far', 'ge': 'strict'}
    for M in ALL_SIZES:
        for bug, family in named.items():
            assert any(not np.array_equal(c.expected(), S.planted_scan(c, bug)) for c in S.nms_family(family, M)), (M, bug)
        case = S.counts_cases(M)[2][1]
        assert not np.array_equal(case.expected(), S.planted_scan(case, 'past_counts')), M


def test_builders_hold_their_preconditions_at_every_size():
    """nms_family asserts chunk, bit, parity and kept-rank of every planted row while it builds; here: what the families
    cover together"""
    for M in ALL_SIZES:
        far = S.nms_family('far', M)[0]
        nchunks = (M + 63) // 64
        want = [d for d in S.FAR_DISTANCES + (S.WIDE_DISTANCES if M in S.WIDE_SIZES else ()) if d <= nchunks - 1]
        assert {p['d'] for p in far.pairs} == set(want), M
        assert {p['bit'] for p in far.pairs} == set(S.VICTIM_BITS)
        for d in want:
            if d <= nchunks - 3:                 # room for an even and an odd suppressor chunk before a full victim chunk
                have = {(p['cls'], p['parity']) for p in far.pairs if p['d'] == d}
                assert {('def', 0), ('def', 1), ('imm', 0), ('imm', 1)} <= have, (M, d, have)
        assert any(p['cls'] == 'mid' and p['d'] >= 3 for p in far.pairs)       # deferred in <3, 2>, immediate in the wide scan
        slots = {(p['victim'] // 64) >> 6 for p in far.pairs}
        assert slots == set(range((nchunks + 63) // 64)), (M, slots)          # every removed-word slot owns a victim
        chain = S.nms_family('chain', M)[0]
        assert {(c['dab'], c['dbc']) for c in chain.chains} >= {(a, b) for a in (0, 1, 2, 3) for b in (0, 1, 3)}
        assert far.boxes().max() < 2 ** 24
        assert S.scan_name(M) == (S.SCAN_WIDE if M in S.WIDE_SIZES else S.SCAN_NARROW)
    assert S.nms_family('far', 32768)[0].boxes().max() <= 1048208


def _cpu_rows(case):
    out = []
    for lvl in range(len(case.levels)):
        rows = case.rows(lvl).sigmoid().numpy()
        out += [(r, min(case.nms_pre, len(r))) for r in rows]
    return out


@pytest.mark.parametrize('bug,name', [('unstable', 'all_equal/k500'), ('cut_last', 'straddle')])
def test_planted_topk_changes_its_named_case(bug, name):
    case = next(c for c in S.topk_cases() if c.name == name)
    assert any(not np.array_equal(S.stable_topk(r, k), S.planted_topk(r, k, bug)) for r, k in _cpu_rows(case))
    for r, k in _cpu_rows(case):                 # the planted selections are still k of the right scores
        assert np.array_equal(np.sort(r[S.planted_topk(r, k, bug)]), np.sort(r[S.stable_topk(r, k)]))


def test_topk_and_merge_builders():
    names = {c.name.split('/')[0] for c in S.topk_cases()}
    assert names == {'all_equal', 'straddle', 'edges', 'ones', 'zeros', 'low_bits', 'rows48', 'k16384'}
    ones = next(c for c in S.topk_cases() if c.name == 'ones')
    assert all((r == 1.0).sum() > k for r, k in _cpu_rows(ones))
    zeros = next(c for c in S.topk_cases() if c.name == 'zeros')
    assert all(0 < (r > 0).sum() < k and (r == 0).sum() > 0 for r, k in _cpu_rows(zeros))
    tiny = S.tiny_case()
    assert tiny.levels[0].dtype == torch.float32 and tiny.rows().shape == (2, 3 * 1089)
    for shape, ks in S.MERGE_SHAPES.items():
        for mode in S.VALID_MODES:
            c = S.merge_case(shape, mode)
            first = 0
            for k in ks:                         # every level stably descending
                lv = c.scores[:, first:first + k]
                assert (lv[:, 1:] <= lv[:, :-1]).all()
                first += k
    assert sum(S.MERGE_SHAPES['lds_limit']) == S.MERGE_MAX_ROWS and len(S.MERGE_SHAPES['eight']) == 8
    assert S.DECODE_OPERANDS['pow2'] == ((0.1, -0.2, 0.05, -0.05), (0.5, 0.5, 0.25, 0.25))
    for operands in S.DECODE_OPERANDS:           # (the builder asserts which set tells a fused multiply-add apart)
        lv, lim = S.decode_case(operands)
        assert len(lv) == 3 and lim.shape == (3, 2) and len({tuple(r) for r in lim.tolist()}) == 3


# ================================================================================================================ NMS
def _nms(dev, boxes, counts, thr, max_keep, n_rows=None, ws_bytes=None):
    """one oadg_nms_batched launch on a workspace and keep buffers full of 0xFF bytes -> (rc, keep, keep_cnt) on the host"""
    from oadg_amd import _lib
    L = _lib.lib()
    b = torch.as_tensor(np.ascontiguousarray(boxes, np.float32)).to(dev)
    n_img, Mmax = b.shape[0], (b.shape[1] if n_rows is None else n_rows)
    cnt = torch.tensor(list(counts), dtype=torch.int32, device=dev)
    nbytes = L.oadg_nms_workspace_bytes(n_img, min(Mmax, S.NMS_MAX_ROWS))
    ws = torch.full((max(nbytes, 8),), 0xFF, dtype=torch.uint8, device=dev)
    keep = torch.full((n_img, b.shape[1]), -1, dtype=torch.int32, device=dev)
    keep_cnt = torch.full((n_img,), -1, dtype=torch.int32, device=dev)
    rc = L.oadg_nms_batched(_lib.ptr(b), _lib.ptr(cnt), n_img, Mmax, float(thr), int(max_keep), _lib.ptr(ws),
                            nbytes if ws_bytes is None else ws_bytes, _lib.ptr(keep), _lib.ptr(keep_cnt), _lib.stream_ptr())
    if rc == 0:
        _SCANS_LAUNCHED.add(S.scan_name(Mmax))
    return rc, keep.cpu().numpy(), keep_cnt.cpu().numpy()


def _check_case(dev, case):
    assert S.scan_name(case.M) == (S.SCAN_WIDE if case.M > 12288 else S.SCAN_NARROW)
    rc, keep, cnt = _nms(dev, case.boxes()[None], [case.count], case.thr, case.max_keep)
    ref = case.expected()
    assert rc == 0
    assert int(cnt[0]) == len(ref), (case.name, int(cnt[0]), len(ref))
    got = keep[0, :len(ref)].astype(np.int64)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (case.name, 'first difference at', int(bad[0]), int(got[bad[0]]), int(ref[bad[0]]))


@gpu
@pytest.mark.parametrize('M', ALL_SIZES)
@pytest.mark.parametrize('family', FAMILIES)
def test_nms_family(dev, family, M):
    for case in S.nms_family(family, M):
        _check_case(dev, case)


@gpu
@pytest.mark.parametrize('M', (1, 63, 64, 65, 12288, 12289))
def test_nms_disjoint(dev, M):
    """every row kept: 64 kept rows per chunk (two deferred and six immediate rounds); max_keep 0 and M + 5 mean all"""
    cases = S.nms_family('disjoint', M)
    assert [c.max_keep for c in cases] == [-1, 1, 64, 65, 1000, M, M + 5]
    for case in cases + [cases[0].with_(f'disjoint/{M}/keep0', max_keep=0)]:
        _check_case(dev, case)
        if case.max_keep in (-1, 0, M, M + 5):
            assert len(case.expected()) == M


@gpu
@pytest.mark.parametrize('Mmax', (4497, 16385))
def test_nms_partial_counts_on_a_dirty_workspace(dev, Mmax):
    """four images, counts (0, 1, Mmax, Mmax - 63), rows past each count are copies of row 0; the mask kernel writes only
    the words of valid rows at or right of the diagonal and the launcher skips the memset"""
    boxes, counts, cases = S.counts_cases(Mmax)
    assert counts == (0, 1, Mmax, Mmax - 63)
    for i, n in enumerate(counts):
        assert np.array_equal(boxes[i, n:], np.broadcast_to(boxes[i, 0], (Mmax - n, 4)))
    rc, keep, cnt = _nms(dev, boxes, counts, 0.7, -1)
    assert rc == 0
    for i, case in enumerate(cases):
        ref = case.expected()
        assert int(cnt[i]) == len(ref), (case.name, int(cnt[i]), len(ref))
        assert np.array_equal(keep[i, :len(ref)].astype(np.int64), ref), case.name
    assert int(cnt[0]) == 0 and keep[1, 0] == 0 and int(cnt[1]) == 1


@gpu
def test_nms_limits_and_both_scan_instantiations(dev):
    one = S.nms_family('disjoint', 64)[0].boxes()[None]
    rc, _, cnt = _nms(dev, one, [64], 0.7, -1, n_rows=S.NMS_MAX_ROWS + 1)
    assert rc == OADG_EARG and int(cnt[0]) == -1                         # nothing ran
    rc, _, cnt = _nms(dev, one, [64], 0.7, -1, ws_bytes=64 * 8 - 1)
    assert rc == OADG_ESIZE and int(cnt[0]) == -1
    for M in (12288, 12289, S.NMS_MAX_ROWS):                              # the threshold between the two scans, the limit
        _check_case(dev, S.nms_family('disjoint', M)[0])
    assert _SCANS_LAUNCHED == {S.SCAN_NARROW, S.SCAN_WIDE}
    assert {S.scan_name(M) for M in S.NARROW_SIZES} == {S.SCAN_NARROW} and {S.scan_name(M) for M in S.WIDE_SIZES} == {S.SCAN_WIDE}


# ============================================================================================================== top-k
def _layout(dev, t, layout):
    """the level as the kernel gets it: fp32 NCHW, or a bf16 channel slice of a wider channels_last tensor (one more image
    and 16 channels of other values around it)"""
    I, A = t.shape[:2]
    if layout == 'f32_nchw':
        return t.to(dev).contiguous()
    g = torch.Generator().manual_seed(int(t.numel()))
    wide = (torch.randn((I + 1, 16) + tuple(t.shape[2:]), generator=g) * 4).bfloat16()
    wide[:I, 2:2 + A] = t.bfloat16()
    wide = wide.to(dev).contiguous(memory_format=torch.channels_last)
    return wide[:, 2:2 + A]


def _topk(dev, cls, dims, n_img, nms_pre):
    from oadg_amd import _lib
    L = _lib.lib()
    nl = len(dims)
    ks = [min(nms_pre, h * w * a) for h, w, a in dims]
    sc = [torch.full((n_img, k), -7.0, dtype=torch.float32, device=dev) for k in ks]
    ix = [torch.full((n_img, k), -7, dtype=torch.int64, device=dev) for k in ks]
    level_n = (ctypes.c_int * nl)(*[h * w * a for h, w, a in dims])
    nbytes = L.oadg_rpn_topk_workspace_bytes(level_n, nl, n_img, nms_pre)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    strides = (ctypes.c_long * (4 * nl))(*[int(v) for c in cls for v in c.stride()])
    dims_c = (ctypes.c_int * (3 * nl))(*[v for d in dims for v in d])
    rc = L.oadg_rpn_topk((ctypes.c_void_p * nl)(*[c.data_ptr() for c in cls]), strides, dims_c,
                         0 if cls[0].dtype == torch.float32 else 1, nl, n_img, nms_pre,
                         (ctypes.c_void_p * nl)(*[t.data_ptr() for t in sc]),
                         (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ix]), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    return rc, sc, ix, ks


def _check_topk(dev, case, layout):
    n_img = case.levels[0].shape[0]
    cls = [_layout(dev, t, layout) for t in case.levels]
    rc, sc, ix, ks = _topk(dev, cls, case.dims, n_img, case.nms_pre)
    assert rc == 0, (case.name, rc)
    for l, c in enumerate(cls):
        ref = c[:n_img].float().permute(0, 2, 3, 1).reshape(n_img, -1).sigmoid()
        rs, ri = ref.sort(dim=1, descending=True, stable=True)
        for i in range(n_img):                   # row by row
            nbad = int((sc[l][i] != rs[i, :ks[l]]).sum())
            assert torch.equal(sc[l][i], rs[i, :ks[l]]), (case.name, layout, 'scores', l, i, nbad)
            nbad = int((ix[l][i] != ri[i, :ks[l]]).sum())
            assert torch.equal(ix[l][i], ri[i, :ks[l]]), (case.name, layout, 'indices', l, i, nbad)


@gpu
@pytest.mark.parametrize('layout', ('f32_nchw', 'bf16_slice'))
@pytest.mark.parametrize('name', [c.name for c in S.topk_cases()])
def test_topk_equals_sigmoid_and_stable_sort(dev, name, layout):
    _check_topk(dev, next(c for c in S.topk_cases() if c.name == name), layout)


@gpu
def test_topk_tiny_scores(dev):
    """logits -104 ... -87: 1 / (1 + e^-x) is subnormal below -87.34 and, in fp32, 0 once e^-x overflows (below -88.72).
    The contract is torch's sigmoid on the device: equal scores (bit for bit, subnormals kept, not flushed) and the
    stable order of the large tie group at 0.0, which k = 2000 cuts."""
    case = S.tiny_case()
    ref = case.rows().to(dev).sigmoid()
    sub = int(((ref > 0) & (ref < torch.finfo(torch.float32).tiny)).sum())
    print('tiny: subnormal reference scores', sub, 'zero', int((ref == 0).sum()), 'of', ref.numel())
    x = case.rows().double()
    lo, hi = -float(np.log(np.finfo(np.float32).max)), float(np.log(np.finfo(np.float32).tiny))       # -88.72, -87.34
    assert sub > 0 and abs(sub - int(((x > lo) & (x < hi)).sum())) <= 12              # (one step of 1/64 at either end)
    assert int((ref > 0).sum()) < case.nms_pre < ref.shape[1]
    _check_topk(dev, case, 'f32_nchw')


@gpu
def test_topk_limits(dev):
    """one past each limit returns OADG_EARG and writes nothing: nms_pre = 16,385 on a row of 20,000; 49 rows"""
    big = next(c for c in S.topk_cases() if c.name == 'k16384')
    cls = [_layout(dev, big.levels[0], 'f32_nchw')]
    rc, sc, ix, _ = _topk(dev, cls, big.dims, 1, 16385)
    assert rc == OADG_EARG and bool((sc[0] == -7).all()) and bool((ix[0] == -7).all())
    levels = [torch.zeros((7, 3, 1, 1)) for _ in range(7)]
    cls = [_layout(dev, t, 'f32_nchw') for t in levels]
    rc, sc, ix, _ = _topk(dev, cls, [(1, 1, 3)] * 7, 7, 2)
    assert rc == OADG_EARG and all(bool((s == -7).all()) for s in sc)
    rc, sc, ix, _ = _topk(dev, cls[:6], [(1, 1, 3)] * 6, 7, 2)            # 42 rows: fine
    assert rc == 0 and all(bool((s == 0.5).all()) for s in sc) and all(bool((i == torch.arange(2, device=dev)).all()) for i in ix)


# =============================================================================================== merge, decode, gather
def _levels(ks, fill=None):
    from oadg_amd import _lib
    levels = (_lib.RpnLevel * len(ks))()
    first = 0
    for l, k in enumerate(ks):
        levels[l].k, levels[l].first = int(k), first
        if fill is not None:
            fill(levels[l], l)
        first += int(k)
    return levels, first


def _order(dev, ks, props, scores, valid):
    from oadg_amd import _lib
    L = _lib.lib()
    levels, M = _levels(ks)
    n_img = scores.shape[0]
    bs = torch.full((n_img, M, 4), float('nan'), dtype=torch.float32, device=dev)
    order = torch.full((n_img, M), -1, dtype=torch.int32, device=dev)
    counts = torch.full((n_img,), -1, dtype=torch.int32, device=dev)
    mx = torch.full((n_img,), float('nan'), dtype=torch.float32, device=dev)
    rc = L.oadg_rpn_order(levels, len(ks), n_img, _lib.ptr(props), _lib.ptr(scores), _lib.ptr(valid), _lib.ptr(bs),
                          _lib.ptr(order), _lib.ptr(counts), _lib.ptr(mx), _lib.stream_ptr())
    return rc, bs, order, counts, mx


def _order_reference(ks, props, scores, valid):
    """the tensor expressions of RPNHead.get_bboxes"""
    n_img = scores.shape[0]
    ids = torch.cat([scores.new_full((k,), l, dtype=torch.long) for l, k in enumerate(ks)])[None].expand(n_img, -1)
    v = valid.bool()
    mx = torch.where(v[..., None], props, props.new_zeros(())).amax(dim=(1, 2))
    offs = ids.to(props) * (mx + 1)[:, None]
    key = torch.where(v, scores, scores.new_full((), -1.0))
    order = key.sort(dim=1, descending=True, stable=True)[1]
    boxes_sorted = torch.gather(props + offs[..., None], 1, order[..., None].expand(-1, -1, 4))
    return boxes_sorted, order, v.sum(dim=1).int(), mx


@gpu
@pytest.mark.parametrize('mode', S.VALID_MODES)
@pytest.mark.parametrize('shape', list(S.MERGE_SHAPES))
def test_merge_equals_the_stable_sort(dev, shape, mode):
    from oadg_amd import _lib
    case = S.merge_case(shape, mode)
    props, scores, valid = case.props.to(dev), case.scores.to(dev), case.valid.to(dev)
    rc, bs, order, counts, mx = _order(dev, case.ks, props, scores, valid)
    assert rc == 0
    rbs, rorder, rcounts, rmx = _order_reference(case.ks, props, scores, valid)
    assert torch.equal(order.long(), rorder), (case.name, int((order.long() != rorder).sum()))
    assert torch.equal(counts, rcounts) and torch.equal(mx, rmx)
    assert torch.equal(bs, rbs), (case.name, int((bs != rbs).any(-1).sum()))
    if mode in ('none', 'one_image_clear'):      # an image without a valid candidate: NMS and gather on nothing
        L = _lib.lib()
        n_img, M = scores.shape
        assert int(counts[1]) == 0 and float(mx[1]) == 0.0
        nbytes = L.oadg_nms_workspace_bytes(n_img, M)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
        keep = torch.full((n_img, M), -1, dtype=torch.int32, device=dev)
        kc = torch.full((n_img,), -1, dtype=torch.int32, device=dev)
        assert L.oadg_nms_batched(_lib.ptr(bs), _lib.ptr(counts), n_img, M, 0.7, 1000, _lib.ptr(ws), nbytes, _lib.ptr(keep),
                                  _lib.ptr(kc), _lib.stream_ptr()) == 0
        P = min(1000, M)
        dets = torch.full((n_img, P, 5), float('nan'), dtype=torch.float32, device=dev)
        assert L.oadg_rpn_gather(n_img, M, P, _lib.ptr(props), _lib.ptr(scores), _lib.ptr(order), _lib.ptr(keep),
                                 _lib.ptr(kc), _lib.ptr(dets), _lib.stream_ptr()) == 0
        assert int(kc[1]) == 0
        empty = torch.tensor([0.0, 0.0, 0.0, 0.0, -1.0], device=dev).expand(P, 5)
        assert torch.equal(dets[1], empty)
        for i in range(n_img if M <= 4000 else 0):          # (the dense oracle: small shapes only)
            ref = ONMS.nms_sorted(bs[i, :int(counts[i])].cpu().numpy(), 0.7, 1000)
            assert int(kc[i]) == len(ref) and np.array_equal(keep[i, :len(ref)].cpu().numpy(), ref)


@gpu
def test_merge_one_past_the_lds_limit_is_an_argument_error(dev):
    M = S.MERGE_MAX_ROWS + 1
    props = torch.zeros((1, M, 4), device=dev)
    scores = torch.zeros((1, M), device=dev)
    valid = torch.ones((1, M), dtype=torch.uint8, device=dev)
    rc, _, order, counts, _ = _order(dev, (M,), props, scores, valid)
    assert rc == OADG_EARG and int(counts[0]) == -1 and bool((order == -1).all())


@gpu
@pytest.mark.parametrize('min_size', (8.0, -1.0))
@pytest.mark.parametrize('layout', ('f32_nchw', 'bf16_slice'))
@pytest.mark.parametrize('operands', list(S.DECODE_OPERANDS))
def test_decode_equals_the_coder(dev, operands, layout, min_size):
    """means / stds that are not 0 / 1 (with stds that are no powers of two a fused or reordered d * std + mean changes
    bits), deltas at and beyond +/- log(1000 / 16), boxes wholly outside the image, per-image limits:
    DeltaXYWHBBoxCoder.decode + the clip and size test of get_bboxes, bit for bit"""
    from oadg_amd import _lib
    from oadg_amd.core.bbox import DeltaXYWHBBoxCoder
    L = _lib.lib()
    lv, lim = S.decode_case(operands)
    MEANS, STDS = S.DECODE_OPERANDS[operands]
    n_img = lim.shape[0]
    dl = [_layout(dev, l['deltas'], layout) for l in lv]
    an = [l['anchors'].to(dev).contiguous() for l in lv]
    ix = [l['index'].to(dev).contiguous() for l in lv]
    sc = [l['scores'].to(dev).contiguous() for l in lv]

    def fill(s, l):
        s.deltas, s.anchors, s.scores, s.index = dl[l].data_ptr(), an[l].data_ptr(), sc[l].data_ptr(), ix[l].data_ptr()
        s.sN, s.sC, s.sH, s.sW = (int(v) for v in dl[l].stride())
        s.H, s.W, s.A = lv[l]['dims']
        s.dtype = 0 if dl[l].dtype == torch.float32 else 1
    levels, M = _levels([l['k'] for l in lv], fill)
    props = torch.full((n_img, M, 4), float('nan'), dtype=torch.float32, device=dev)
    scores = torch.full((n_img, M), float('nan'), dtype=torch.float32, device=dev)
    valid = torch.full((n_img, M), 7, dtype=torch.uint8, device=dev)
    limd = lim.to(dev)
    means, stds = (ctypes.c_float * 4)(*MEANS), (ctypes.c_float * 4)(*STDS)
    max_ratio = float(np.float32(np.abs(np.log(16 / 1000))))
    assert L.oadg_rpn_decode(levels, len(lv), n_img, means, stds, max_ratio, _lib.ptr(limd), 1, min_size, _lib.ptr(props),
                             _lib.ptr(scores), _lib.ptr(valid), _lib.stream_ptr()) == 0
    coder = DeltaXYWHBBoxCoder(target_means=MEANS, target_stds=STDS)
    d_l, a_l = [], []
    for l in range(len(lv)):
        d = dl[l][:n_img].float().permute(0, 2, 3, 1).reshape(n_img, -1, 4)
        top = ix[l]
        d_l.append(torch.gather(d, 1, top[..., None].expand(-1, -1, 4)))
        a_l.append(torch.gather(an[l][None].expand(n_img, -1, -1), 1, top[..., None].expand(-1, -1, 4)))
    deltas, anchors = torch.cat(d_l, 1), torch.cat(a_l, 1)
    ref = coder.decode(anchors.reshape(-1, 4), deltas.reshape(-1, 4), max_shape=None).view(n_img, M, 4)
    raw = ref
    ref = torch.minimum(ref.clamp(min=0), limd.repeat(1, 2)[:, None, :])
    w, h = ref[..., 2] - ref[..., 0], ref[..., 3] - ref[..., 1]
    rvalid = ((w > min_size) & (h > min_size)) if min_size >= 0 else torch.ones_like(w, dtype=torch.bool)
    # the case does what it says: clamped ratios on both sides, boxes wholly outside, both flags
    dwh = deltas[..., 2:] * torch.tensor(STDS[2:], device=dev) + torch.tensor(MEANS[2:], device=dev)
    assert int((dwh > max_ratio).sum()) > 50 and int((dwh < -max_ratio).sum()) > 50
    assert int((raw[..., 2] < 0).sum()) > 10 and int((raw[..., 0] > limd[:, None, 0]).sum()) > 10
    assert torch.equal(props, ref), int((props != ref).any(-1).sum())
    assert torch.equal(scores, torch.cat(sc, 1))
    assert torch.equal(valid.bool(), rvalid) and int(valid.max()) <= 1
    if min_size >= 0:
        assert 0 < int(rvalid.sum()) < rvalid.numel()


@gpu
def test_gather_pads_and_clamps(dev):
    """rows past keep_cnt are (0, 0, 0, 0, -1); keep indices outside [0, M) read row 0 / M - 1, as the tensor path's clamp"""
    from oadg_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(21)
    n_img, M, P = 4, 700, 300
    props = torch.rand((n_img, M, 4), generator=g).mul(500).to(dev)
    scores = torch.rand((n_img, M), generator=g).to(dev)
    order = torch.stack([torch.randperm(M, generator=g) for _ in range(n_img)]).int().to(dev)
    keep = torch.stack([torch.randperm(M, generator=g) for _ in range(n_img)]).int()
    keep[:, 3], keep[:, 10], keep[:, 11], keep[:, 200] = -1, M, 2 ** 31 - 1, -2 ** 31
    keep = keep.to(dev)
    keep_cnt = torch.tensor([0, 37, P, M], dtype=torch.int32, device=dev)
    dets = torch.full((n_img, P, 5), float('nan'), dtype=torch.float32, device=dev)
    assert L.oadg_rpn_gather(n_img, M, P, _lib.ptr(props), _lib.ptr(scores), _lib.ptr(order), _lib.ptr(keep),
                             _lib.ptr(keep_cnt), _lib.ptr(dets), _lib.stream_ptr()) == 0
    kidx = keep[:, :P].long().clamp(0, M - 1)
    sel = torch.gather(order.long(), 1, kidx)
    live = torch.arange(P, device=dev)[None, :] < keep_cnt[:, None]
    pb = torch.gather(props, 1, sel[..., None].expand(-1, -1, 4))
    ps = torch.gather(scores, 1, sel)
    ref = torch.cat([torch.where(live[..., None], pb, pb.new_zeros(())), torch.where(live, ps, ps.new_full((), -1.0))[..., None]], 2)
    assert torch.equal(dets, ref)
    pad = torch.tensor([0.0, 0.0, 0.0, 0.0, -1.0], device=dev)
    assert torch.equal(dets[0], pad.expand(P, 5)) and torch.equal(dets[1, 37:], pad.expand(P - 37, 5))


# ==================================================================================================== through the head
def _head(dev, strides, scales, nms_pre, max_per_img, min_bbox_size):
    from oadg_amd import Config
    from oadg_amd.dense_heads import RPNHead
    test_cfg = Config(dict(nms_pre=nms_pre, max_per_img=max_per_img, nms=dict(type='nms', iou_threshold=0.7),
                           min_bbox_size=min_bbox_size))
    return RPNHead(in_channels=256, feat_channels=256,
                   anchor_generator=dict(type='AnchorGenerator', scales=scales, ratios=[0.5, 1.0, 2.0], strides=strides),
                   bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]),
                   loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                   loss_bbox=dict(type='L1Loss', loss_weight=1.0), test_cfg=test_cfg).to(dev)


def _head_outputs(dev, n, H, W, strides, A, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    cs, bp = [], []
    for s in strides:
        h, w = -(-H // s), -(-W // s)
        cs.append((torch.randn(n, A, h, w, device=dev, generator=g) * 8).round() / 4)        # exact ties
        bp.append(torch.randn(n, 4 * A, h, w, device=dev, generator=g) * 0.4)
    return cs, bp


def _both_paths(head, cs, bp, metas, calls=None):
    from oadg_amd.dense_heads import RPNHead
    out = {}
    for fused in (True, False):
        RPNHead.FUSED_PROPOSALS = fused
        try:
            if calls is not None:
                calls.clear()
            out[fused, True] = head.get_bboxes(cs, bp, img_metas=metas, padded=True)
            out[fused, False] = head.get_bboxes(cs, bp, img_metas=metas, padded=False)
            if calls is not None and fused:
                out['calls'] = list(calls)
        finally:
            RPNHead.FUSED_PROPOSALS = True
    for padded in (True, False):
        a, b = out[True, padded], out[False, padded]
        assert len(a) == len(b) == len(metas)
        for x, y in zip(a, b):
            assert x.shape == y.shape and torch.equal(x, y), (padded, tuple(x.shape), tuple(y.shape))
    return out


@gpu
def test_head_image_without_a_valid_candidate(dev):
    """one image of the batch is smaller than min_bbox_size: every candidate of it is invalid, counts = 0, zero proposals"""
    strides = [4, 8, 16, 32, 64]
    head = _head(dev, strides, [8], 2000, 1000, 16)
    cs, bp = _head_outputs(dev, 3, 128, 128, strides, 3, 31)
    metas = [dict(img_shape=s, pad_shape=(128, 128, 3)) for s in ((128, 128, 3), (10, 12, 3), (100, 128, 3))]
    out = _both_paths(head, cs, bp, metas)
    assert out[True, False][1].shape == (0, 5) and out[False, False][1].shape == (0, 5)
    assert bool((out[True, True][1][:, 4] == -1).all()) and bool((out[True, True][1][:, :4] == 0).all())
    assert out[True, False][0].shape[0] > 0 and out[True, False][2].shape[0] > 0


@gpu
@pytest.mark.parametrize('which', ('rows49', 'k16385'))
def test_head_takes_the_sort_path_past_the_topk_limits(dev, which, monkeypatch):
    """49 (image, level) rows, or nms_pre = 16,385 on a level of 17,280 anchors: get_bboxes must not call oadg_rpn_topk,
    still runs the fused decode / merge / NMS / gather after torch.sort, and equals the tensor path"""
    from oadg_amd import _lib
    L = _lib.lib()
    calls = []
    for name in ('oadg_rpn_topk', 'oadg_rpn_decode', 'oadg_rpn_order', 'oadg_rpn_gather'):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    if which == 'rows49':
        strides = [4, 8, 16, 32, 64, 128, 256]
        head = _head(dev, strides, [8], 100, 50, 0)
        cs, bp = _head_outputs(dev, 7, 64, 64, strides, 3, 32)
        metas = [dict(img_shape=(64, 64, 3))] * 7
        assert len(cs) * 7 == 49
    else:
        head = _head(dev, [16], [2, 4, 8, 16, 32], 16385, 300, 0)
        cs, bp = _head_outputs(dev, 1, 384, 768, [16], 15, 33)
        metas = [dict(img_shape=(384, 768, 3))]
        assert cs[0][0].numel() == 17280
    out = _both_paths(head, cs, bp, metas, calls)
    assert out['calls'] == ['oadg_rpn_decode', 'oadg_rpn_order', 'oadg_rpn_gather'] * 2, out['calls']
    if which == 'k16385':
        assert S.scan_name(16385) == S.SCAN_WIDE and out[True, True][0].shape == (300, 5)
    # within the limits the same head does call the select kernels
    calls.clear()
    n = 6 if which == 'rows49' else 1
    head.test_cfg.nms_pre = min(head.test_cfg.nms_pre, 16384)
    head.get_bboxes([c[:n] for c in cs], [b[:n] for b in bp], img_metas=metas[:n], padded=True)
    assert calls[0] == 'oadg_rpn_topk', calls
