"""OA-Mix's region ops, histogram / LUT kernels and final mix, ONE OP AT A TIME through the C ABI of csrc/oamix.hip on the
degenerate images of tests/oamix_cases.py: saturated, flat, binary and narrow-range channels, images of 1 and 2 pixels
across, pixel counts of every residue mod 4, more than one histogram workgroup, the grid-stride second trip.

Every comparison is np.array_equal on bytes (fp32 / bf16 outputs on their bits); nothing skips.
  A  colour ops, hist, luts, gray_sum, compose layouts and accumulator modes        against Pillow
  B  OADG_OP_WARP_NEG and OADG_OP_BG_WARP with scripted draws                        against oracle OAMixOracle.aug
  C  OAMix._bboxes_only on its three host paths with scripted draws                  against OAMixOracle.bboxes_only
  D  oadg_oamix_final, oadg_oamix_final_tiles, oadg_oamix_normalize                  against OAMixOracle.object_aware_mixing
The CPU tests hold the NumPy restatement of oamix_cases.py to Pillow on every case of A (and its final mix to the oracle on
every case of D), show that each degenerate branch is reached, and plant ten errors that named cases must notice.

Two places where the cases differ from their first description, both because the reference says so:
  * ``one_outlier`` at 17 x 23 has equalize step (391 - 1) // 255 = 1, not 0; step == 0 is asserted at 3 x 3 and 5 x 7
    (8 // 255, 34 // 255) and step == 1, the smallest step that divides, at 17 x 23.
  * at 1 x 9 and 9 x 2 the quarter-resolution mask of a gt box has no rows (H // 4 == 0 or W // 4 == 0): the reference
    cannot resize it (asserted below), so section B runs only the no-box mask variant at these two sizes.

Which compose kernel a launch takes is the launcher's own predicate (W % 4 == 0, 4-byte aligned images, 16-byte aligned
accumulator), restated in ``_compose_kernel_name``.

Measured wall time of the module: 3.3 s for the CPU tests (-m "not gpu", 22 tests), 4.9 s for the GPU tests (-m gpu, 30
tests, 11,141 compose and 1,215 final-mix launches) on one MI355X.
"""
import ctypes
import time
from collections import Counter

import numpy as np
import pytest

import oamix_cases as C
from oracle import cvleaves as cv
from oracle import oamix as OO

gpu = pytest.mark.gpu
LEDGER = dict(kinds=Counter(), kernels=Counter(), finals=Counter())      # what the GPU tests of this module launched
KIND = dict(copy=0, autocontrast=1, equalize=2, posterize=3, solarize=4, image=5, bg_warp=6, warp_neg=7, brightness=8,
            color=9, contrast=10, sharpness=11)


# ============================================================================================================ CPU self-tests
@pytest.mark.parametrize('name', C.IMAGES)
def test_restatement_equals_pillow(name):
    """self-test 1: tables, luma, contrast mean, SMOOTH filter and blend of the restatement against Pillow, whole grid of A"""
    n = 0
    for H, W in C.SIZES_A:
        img = C.image(name, H, W)
        tables = C.luts(img)
        for k, op in enumerate(C.LUT_OPS):
            want, present = C.lut_from_outputs(img, C.pillow_op(op, None, img))
            assert np.array_equal(tables[k][present], want[present]), (name, H, W, op)
        assert C.gray_sum(img) == C.pillow_gray_sum(img), (name, H, W)
        for op, p in C.color_ops():
            assert np.array_equal(C.restated_op(op, p, img), C.pillow_op(op, p, img)), (name, H, W, op, p)
            n += 1
    print(f'{name}: {n} op cases equal Pillow')


def test_restatement_equals_pillow_on_the_large_image():
    img = C.image('noise', *C.SIZE_BIG)
    for op, p in C.color_ops(big=True):
        assert np.array_equal(C.restated_op(op, p, img), C.pillow_op(op, p, img)), (op, p)


def _mix_case(H, W, tlist, shift):
    """(masks, m_oas, scores, units, fg boxes) of one final-mix case"""
    oracle = OO.OAMixOracle()
    units = C.mix_units(len(tlist), shift)
    masks, m_oas, fg = [], [], []
    for (kind, box), (u, score) in zip(tlist, units):
        if kind == 'fg':
            masks.append(oracle.blur_mask(np.array(box, np.float32), H, W))
            fg.append(box)
        else:
            masks.append(OO.OAMixOracle.sharp_mask(box, H, W))
        hi = 0.5 if score <= oracle.score_thresh else 1.0
        m_oas.append(np.float32(0.0 + (hi - 0.0) * u))
    return masks, m_oas, [s for _, s in units], [float(u) for u, _ in units], fg


def _oracle_mix(monkeypatch, img, acc, masks, scores, units, m_beta):
    script = C.Script([float(m_beta)] + units)
    with monkeypatch.context() as mp:
        script.patch_numpy(mp)
        oracle = OO.OAMixOracle()
        out = oracle.object_aware_mixing(img, acc, masks, scores)
    assert script.done(), 'the oracle left scripted draws unused'
    assert [t[1] for t in oracle.trace if t[0] == 'beta'] == [float(m_beta)]
    return np.asarray(out, dtype=np.uint8), out, [t[1] for t in oracle.trace if t[0] == 'm_oa']


_MIX_REF = {}


def _mix_reference(monkeypatch, H, W, tname, m_beta, shift):
    """the oracle's view of one case of D, computed once and shared between the CPU and the GPU tests"""
    key = (H, W, tname, m_beta, shift)
    if key not in _MIX_REF:
        img, acc = C.mix_inputs(H, W)
        tlist = dict(C.mix_targets(H, W))[tname]
        masks, m_oas, scores, units, fg = _mix_case(H, W, tlist, shift)
        want, _, drawn = _oracle_mix(monkeypatch, img, acc, masks, scores, units, m_beta)
        assert drawn == [float(v) for v in m_oas], 'the weights the device is given are the ones the oracle drew'
        want.setflags(write=False)
        _MIX_REF[key] = (want, masks, m_oas, fg, tlist)
    return _MIX_REF[key]


@pytest.mark.parametrize('H,W', C.SIZES_MIX)
def test_final_mix_restatement_equals_the_oracle(monkeypatch, H, W):
    img, acc = C.mix_inputs(H, W)
    clipped = 0
    for tname, _ in C.mix_targets(H, W):
        for m_beta in C.M_BETAS:
            for shift in range(3):
                want, masks, m_oas, _, _ = _mix_reference(monkeypatch, H, W, tname, m_beta, shift)
                got, c = C.final_mix(img, acc, masks, m_oas, m_beta)
                clipped += c
                assert np.array_equal(got, want), (H, W, tname, m_beta, shift, int((got != want).sum()))
    assert clipped > 0, 'no accumulator case clipped'


def test_each_degenerate_branch_is_reached(monkeypatch):
    """self-test 2, on the reference side"""
    ident = np.arange(256).astype(np.uint8)
    for H, W in C.SIZES_A:
        img = C.image('flat', H, W)
        for op in C.LUT_OPS:                                  # hi <= lo, one non-empty bin
            assert np.array_equal(C.pillow_op(op, None, img), img)
        assert all(C.equalize_step(h) is None for h in C.hist3(img))
        assert np.array_equal(C.luts(img), np.broadcast_to(ident, (2, 3, 256)))
    steps = {s: [C.equalize_step(h) for h in C.hist3(C.image('one_outlier', *s))] for s in ((3, 3), (5, 7), (17, 23))}
    assert steps[(3, 3)] == [0, None, 0] and steps[(5, 7)] == [0, None, 0] and steps[(17, 23)] == [1, None, 1]
    for s in ((3, 3), (5, 7)):                                # step == 0: Pillow's identity, although two bins are filled
        img = C.image('one_outlier', *s)
        assert np.array_equal(C.pillow_op('equalize', None, img), img)
    img = C.image('noise', 17, 23)
    assert np.array_equal(C.pillow_op('solarize', 256, img), img)
    assert not np.array_equal(C.pillow_op('solarize', 255, img), img)
    assert not C.pillow_op('posterize', 0, img).any() and C.posterize_mask(0) == 0 and C.posterize_mask(4) == 0xF0
    assert all((C.image(n, 17, 23) == 255).any() for n in ('noise', 'flat', 'sat_checker', 'binary_noise', 'ramp'))
    chk = C.image('sat_checker', 17, 23)
    assert C.blend(np.zeros_like(chk), chk, 1.9)[1] >= 100    # brightness 1.9: 255 -> 484.5, clamped
    assert C.blend(np.zeros_like(chk), chk, 1.0000001)[1] > 0 and C.blend(np.zeros_like(chk), chk, 1.0)[1] == 0
    flat = C.image('flat', 17, 23)
    assert C.smooth(flat)[1] >= 1 and C.smooth(flat[..., :2])[1] == 0      # channel 2 = 255: 0.5 + 255 >= 255
    assert np.array_equal(C.pillow_op('sharpness', 0.5, flat), flat)
    for H, W in C.SIZES_MIX:                                  # the accumulator of D clips
        img, acc = C.mix_inputs(H, W)
        assert (acc == 0).any() and (acc == 255).any() and ((acc > 255) & (img == 255)).any()
        _, raw, _ = _oracle_mix(monkeypatch, img, acc, [], [], [], 1.0)
        assert np.asarray(raw).max() == 255.0 and (acc > 255).any()
    assert [h * w % 4 for h, w in C.SIZES_MAIN] == [1, 3, 3, 0, 1] and C.SIZE_MULTI[0] * C.SIZE_MULTI[1] % 4 == 3
    assert C.SIZE_BIG[0] * C.SIZE_BIG[1] > 8192 * 256 and C.SIZE_BIG[1] % 4
    for H, W in C.SIZES_THIN:                                 # no quarter-resolution rows: the reference has no mask here
        with pytest.raises(ZeroDivisionError):
            cv.box_mask_profiles(np.array([0, 0, W, H], np.float32), H, W, 4, 0.3)
        assert [n for n, _ in C.mask_variants(H, W)] == ['no_box']
    assert [n for n, _ in C.mask_variants(17, 23)] == ['no_box', 'full_box', 'three_boxes']


PLANTED_CASES = {
    'eq_step0': ('one_outlier', 5, 7, 'equalize', None),
    'ac_round': ('ramp', 17, 23, 'autocontrast', None),
    'blend_clamp': ('sat_checker', 17, 23, 'brightness', 1.9),
    'sharp_border': ('noise', 17, 23, 'sharpness', 0.5),
    'mean_half': ('sat_checker', 33, 64, 'contrast', 0.5),
    'sol_le': ('sat_checker', 5, 7, 'solarize', 255),
    'post_bit': ('noise', 5, 7, 'posterize', 4),
    'hist_tail': ('one_outlier', 5, 7, 'autocontrast', None),
}


@pytest.mark.parametrize('error', C.PLANTED)
def test_planted_errors_are_caught(monkeypatch, error):
    """self-test 3: the error, made in the restatement, changes at least one byte of its named case"""
    assert set(PLANTED_CASES) | {'rect_right4', 'rest_moa'} == set(C.PLANTED)
    if error in PLANTED_CASES:
        name, H, W, op, p = PLANTED_CASES[error]
        img = C.image(name, H, W)
        want = C.pillow_op(op, p, img)
        good, bad = C.restated_op(op, p, img), C.restated_op(op, p, img, planted=(error,))
        if error == 'hist_tail':
            assert not np.array_equal(C.hist3(img, (error,)), C.hist3(img))
    elif error == 'rect_right4':
        img = C.image('noise', 33, 64)
        outs = [C.pillow_op('posterize', 0, img), C.pillow_op('solarize', 1, img), img]
        rects = dict(C.layouts(33, 64))['top_right+bottom_left']
        assert any(r[2] % 4 for r in rects)
        want = outs[2].copy()
        for k, (x1, y1, x2, y2) in enumerate(rects):
            want[y1:y2, x1:x2] = outs[k][y1:y2, x1:x2]
        good, bad = C.compose(outs, rects), C.compose(outs, rects, planted=(error,))
    else:
        H, W = 33, 64
        img, acc = C.mix_inputs(H, W)
        want, masks, m_oas, _, _ = _mix_reference(monkeypatch, H, W, 'fg_fg_rect', 0.5, 0)
        good, bad = C.final_mix(img, acc, masks, m_oas, 0.5)[0], C.final_mix(img, acc, masks, m_oas, 0.5, (error,))[0]
    assert np.array_equal(good, want)
    changed = int((bad != want).sum())
    print(f'{error}: {changed} bytes differ')
    assert changed >= 1, error


# ============================================================================================================ GPU side
def _lib():
    from oadg_amd import _lib as L
    return L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _up(arr, dev):
    import torch
    return torch.from_numpy(np.array(arr, copy=True, order='C')).to(dev)


def _src_tensor(img, dev, offset):
    """the image on the device; ``offset``: a view that starts one pixel (3 bytes) into its buffer, not 4-byte aligned"""
    import torch
    if not offset:
        t = _up(img, dev)
        assert t.data_ptr() % 4 == 0
        return t, t
    buf = torch.zeros((img.size + 8,), dtype=torch.uint8, device=dev)
    view = buf[3:3 + img.size].view(img.shape)
    view.copy_(_up(img, dev))
    assert view.data_ptr() % 4 == 3
    return view, buf


def _compose_kernel_name(W, src, dst, acc):
    quad = W % 4 == 0 and (src.data_ptr() | dst.data_ptr()) % 4 == 0 and acc.data_ptr() % 16 == 0
    return 'compose4_kernel' if quad else 'compose_kernel'


class _Composer:
    """compose launches on one source image: every launch writes its own slice of one result tensor and one accumulator
    tensor (filled with ``old`` beforehand), both read back once"""

    def __init__(self, dev, img, n_launch, offset=False, union=None):
        import torch
        self.L, self.lib = _lib(), _lib().lib()
        self.img, self.dev = img, dev
        self.H, self.W = img.shape[:2]
        self.src, self._keep = _src_tensor(img, dev, offset)
        self.old = np.random.RandomState(7).uniform(-3, 300, img.shape).astype(np.float32)
        self.dst = torch.full((n_launch,) + img.shape, 0xA5, dtype=torch.uint8, device=dev)
        self.acc = _up(np.broadcast_to(self.old, (n_launch,) + img.shape), dev)
        self.union_f, self.union_u8 = union if union else (None, None)
        self.luts = self.gray = self.other = None
        self.jobs = []

    def tables(self):
        """hist -> luts, gray sum and the OADG_OP_IMAGE operand of this source"""
        import torch
        n = self.H * self.W
        src = _up(self.img, self.dev)                        # (the histogram reads aligned dwords: the aligned copy)
        self.hist = torch.full((768,), -1, dtype=torch.int32, device=self.dev)
        self.luts = torch.full((2 * 768,), 0xEE, dtype=torch.uint8, device=self.dev)
        self.gray = torch.full((1,), -1, dtype=torch.int64, device=self.dev)
        st = self.L.stream_ptr()
        self.L.check(self.lib.oadg_oamix_hist(_ptr(src), n, _ptr(self.hist), st), 'oadg_oamix_hist')
        self.L.check(self.lib.oadg_oamix_luts(_ptr(self.hist), _ptr(self.luts), st), 'oadg_oamix_luts')
        self.L.check(self.lib.oadg_oamix_gray_sum(_ptr(src), n, _ptr(self.gray), st), 'oadg_oamix_gray_sum')
        self.other = _up(C.other_image(self.img), self.dev)
        self._keep = (self._keep, src)

    def region_op(self, name, param):
        op = self.L.RegionOp()
        op.kind = KIND[name]
        if name == 'posterize':
            op.param = C.posterize_mask(param)
        elif name == 'solarize':
            op.param = param
        elif name == 'image':
            op.image = self.other.data_ptr()
        elif name in C.ENHANCERS:
            op.minv[0] = param
            if name == 'contrast':
                op.image = self.gray.data_ptr()
        return op

    def launch(self, ops, rects, mode, w, want, what):
        """ops: three RegionOp (rects 0, 1, outside); want: the expected uint8 image"""
        i = len(self.jobs)
        arr = (self.L.RegionOp * 3)(*ops)
        flat = [int(v) for r in rects for v in r]
        rc = (ctypes.c_int * 8)(*flat, *([0] * (8 - len(flat))))
        dst, acc = self.dst[i], self.acc[i]
        self.L.check(self.lib.oadg_oamix_compose(_ptr(self.src), _ptr(dst), self.H, self.W, arr, rc, len(rects),
                                                 _ptr(self.luts), _ptr(self.union_f), _ptr(self.union_u8), _ptr(acc),
                                                 float(w), mode, self.L.stream_ptr()), 'oadg_oamix_compose')
        LEDGER['kernels'][_compose_kernel_name(self.W, self.src, dst, acc)] += 1
        for op in ops[:len(rects)] + ops[2:]:
            LEDGER['kinds'][op.kind] += 1
        self.jobs.append((want, mode, np.float32(w), what))

    def check(self, stats):
        """read everything back and compare: result bytes, accumulator bits"""
        dst, acc = self.dst[:len(self.jobs)].cpu().numpy(), self.acc[:len(self.jobs)].cpu().numpy()
        for i, (want, mode, w, what) in enumerate(self.jobs):
            bad = int((dst[i] != want).sum())
            assert bad == 0, f'{what}: {bad} of {want.size} bytes differ, first at {np.argwhere(dst[i] != want)[0].tolist()}'
            t = w * dst[i].astype(np.float32)
            wacc = self.old if mode == 0 else (t if mode == 1 else self.old + t)
            assert np.array_equal(acc[i].view(np.int32), wacc.view(np.int32)), f'{what}: accumulator, mode {mode}'
            stats[what.split('|')[0]] += np.array([1, want.size + 4 * want.size])
        self.jobs = []


def _report(title, stats, t0):
    print(f'{title}: {time.time() - t0:.2f} s')
    for k in sorted(stats):
        print(f'  {k:<28s} launches {int(stats[k][0]):6d}   bytes compared {int(stats[k][1]):12d}')


class _Stats(dict):
    def __missing__(self, k):
        self[k] = np.zeros(2, np.int64)
        return self[k]


@gpu
@pytest.mark.parametrize('name', C.IMAGES)
def test_hist_luts_gray_sum(dev, name):
    """oadg_oamix_hist against np.bincount, oadg_oamix_luts against the tables Pillow's results show (at the values the
    image holds), oadg_oamix_gray_sum against the sum of Pillow's convert('L')"""
    t0, stats = time.time(), _Stats()
    for H, W in C.SIZES_A:
        img = C.image(name, H, W)
        cp = _Composer(dev, img, 1)
        cp.tables()
        hist = cp.hist.cpu().numpy().reshape(3, 256)
        want = np.stack([np.bincount(img[..., c].reshape(-1), minlength=256) for c in range(3)])
        assert np.array_equal(hist, want), (name, H, W, 'hist')
        stats['hist'] += (1, hist.nbytes)
        tables = cp.luts.cpu().numpy().reshape(2, 3, 256)
        for k, op in enumerate(C.LUT_OPS):
            table, present = C.lut_from_outputs(img, C.pillow_op(op, None, img))
            assert np.array_equal(tables[k][present], table[present]), (name, H, W, op)
            stats['luts ' + op] += (1, int(present.sum()))
        assert np.array_equal(tables, C.luts(img)), (name, H, W, 'tables at absent values')
        assert int(cp.gray.item()) == C.pillow_gray_sum(img), (name, H, W, 'gray_sum')
        stats['gray_sum'] += (1, 8)
    _report(f'hist / luts / gray_sum on {name}', stats, t0)


def _colour_case(dev, img, offset, stats, big=False):
    """every colour op of A in every layout, three regions per launch, the accumulator modes in turn"""
    H, W = img.shape[:2]
    ops = C.color_ops(big)
    refs = {o: C.pillow_op(o[0], o[1], img) for o in ops}
    lay = [l for l in C.layouts(H, W) if not big or l[0] == 'top_right+bottom_left']
    plan = []
    for li, (lname, rects) in enumerate(lay):
        r = len(rects) + 1
        for g in range((len(ops) + r - 1) // r):
            chunk = [ops[(g * r + j) % len(ops)] for j in range(r)]
            chunk = chunk[li % r:] + chunk[:li % r]
            plan.append((lname, rects, chunk, 2 if big else (g + li) % 3))
    cp = _Composer(dev, img, len(plan), offset)
    cp.tables()
    for i, (lname, rects, chunk, mode) in enumerate(plan):
        slots = chunk[:-1] + [('copy', None)] * (3 - len(chunk)) + chunk[-1:]          # rects 0.., filler, outside
        outs = [refs[o] for o in slots[:len(rects)]] + [None] * (2 - len(rects)) + [refs[slots[2]]]
        want = C.compose(outs, rects)
        what = '+'.join(o[0] for o in chunk) + f'|{lname}|{chunk}|mode {mode}|{img.shape}|offset {offset}'
        cp.launch([cp.region_op(*o) for o in slots], rects, mode, C.acc_weight(i), want, what)
    kern = _compose_kernel_name(W, cp.src, cp.dst[0], cp.acc[0])
    local = _Stats()
    cp.check(local)
    for k, v in local.items():                              # per op: the launches it took part in, the bytes of those launches
        for op in set(k.split('+')):
            stats[op] += v
    stats[f'{kern}: all'] += sum(local.values())


@gpu
@pytest.mark.parametrize('name', C.IMAGES)
def test_colour_ops_in_every_layout_equal_pillow(dev, name):
    """section A: zero, one and two rectangles with a different op per region, 1 x 1 rectangles, rectangles at every image
    corner, edges that are no multiple of 4, both compose kernels, acc_mode 0 / 1 / 2"""
    t0, stats = time.time(), _Stats()
    for H, W in C.SIZES_A:
        for offset in ((False, True) if W % 4 == 0 else (False,)):
            _colour_case(dev, C.image(name, H, W), offset, stats)
    assert {k.split(':')[0] for k in stats if k.endswith(': all')} == {'compose_kernel', 'compose4_kernel'}
    _report(f'colour ops on {name}', stats, t0)


@gpu
def test_compose_kernel_second_grid_stride_trip(dev):
    """1025 x 2047 > 8192 x 256 pixels: the last pixels are the second trip of compose_kernel's grid-stride loop"""
    t0, stats = time.time(), _Stats()
    _colour_case(dev, C.image('noise', *C.SIZE_BIG), False, stats, big=True)
    assert [k for k in stats if k.endswith(': all')] == ['compose_kernel: all']
    _report('large image', stats, t0)


@gpu
def test_the_comparison_notices_one_wrong_parameter(dev):
    """the harness itself: solarize(127) on the device against Pillow's solarize(128) differs exactly at the bytes of value 127"""
    img = C.image('noise', 17, 23)
    assert (img == 127).any()
    cp = _Composer(dev, img, 1)
    cp.tables()
    copy = cp.region_op('copy', None)
    cp.launch([copy, copy, cp.region_op('solarize', 127)], [], 1, 0.5, C.pillow_op('solarize', 128, img), 'solarize|off by one')
    with pytest.raises(AssertionError, match=f'{int((img == 127).sum())} of {img.size} bytes differ'):
        cp.check(_Stats())


@gpu
@pytest.mark.parametrize('name', ('noise', 'sat_checker', 'flat'))
def test_warp_ops_with_scripted_draws_equal_the_oracle(dev, monkeypatch, name):
    """section B: 'invert' for the four (tx, ty) and the five bg_only kinds with both signs at three levels, the draws
    scripted on both sides, the union masks from _ImageState"""
    from oadg_amd.pipelines import oa_mix
    t0, stats = time.time(), _Stats()
    mix = oa_mix.OAMix(version='augmix.all')
    scripts = C.warp_scripts(mix.aug_list)
    assert mix.aug_list == OO.AUG_LISTS['augmix.all'] and len(scripts) == 4 + 5 * 2 * 3
    for H, W in C.SIZES_WARP:
        img = C.image(name, H, W)
        for vname, gts in C.mask_variants(H, W):
            oracle = OO.OAMixOracle(version='augmix.all')
            fg_masks = [oracle.blur_mask(g, H, W) for g in gts]
            refs = []
            for label, draws in scripts:
                s = C.Script(draws)
                with monkeypatch.context() as mp:
                    s.patch_numpy(mp)
                    refs.append(np.asarray(oracle.aug(img, gts, fg_masks), dtype=np.uint8))
                assert s.done(), (label, 'oracle')
            for offset in ((False, True) if W % 4 == 0 else (False,)):
                src, _buf = _src_tensor(img, dev, offset)          # (_buf: the view's storage)
                st = oa_mix._ImageState(src, gts, 4, 0.3)
                cp = _Composer(dev, img, len(scripts), offset, union=(st.union_f, st.union_u8))
                cp.src = src
                for (label, draws), want in zip(scripts, refs):
                    s = C.Script(draws)
                    oa_mix.use_random_state(s)
                    try:
                        op = mix._aug(st, src, dict(n_tmp=0, luts_for=None))
                    finally:
                        oa_mix.use_random_state(None)
                    assert s.done(), (label, 'product')
                    assert op.kind == (KIND['warp_neg'] if label.startswith('invert') else KIND['bg_warp'])
                    copy = cp.region_op('copy', None)
                    what = f'{label.split(" u")[0].split(" tx")[0]}|{label}|{vname}|{img.shape}|offset {offset}'
                    cp.launch([copy, copy, op], [], 0, 0.0, want, what)
                cp.check(stats)
    _report(f'warp ops on {name}', stats, t0)


@gpu
@pytest.mark.parametrize('H,W', C.SIZES_BOX)
@pytest.mark.parametrize('name', ('noise', 'sat_checker'))
def test_bboxes_only_one_kind_at_a_time(dev, monkeypatch, name, H, W):
    """section C: OAMix._bboxes_only against OAMixOracle.bboxes_only, five kinds x both signs x both level extremes x six
    box sets, on the three host paths (plan in C, plan in numpy, one launch pair per box)"""
    from oadg_amd.pipelines import oa_mix
    t0, stats = time.time(), _Stats()
    img = C.image(name, H, W)
    src = _up(img, dev)
    paths = (('plan_c', True, True), ('plan_numpy', False, True), ('per_box', True, False))
    mix = oa_mix.OAMix()
    changed = 0
    for bname, gts in C.box_sets(H, W):
        oracle = OO.OAMixOracle()
        fg_masks = [oracle.blur_mask(g, H, W) for g in gts]
        st = oa_mix._ImageState(src, gts, 4, 0.3)
        for kind in C.GEO_KINDS:
            for u_sign in (C.U_PLUS, C.U_MINUS):
                for u_level in (C.U_LOW, C.U_HIGH):
                    draws = C.box_draws(gts, u_level, u_sign)
                    s = C.Script(draws)
                    with monkeypatch.context() as mp:
                        s.patch_numpy(mp)
                        want = np.asarray(oracle.bboxes_only(img, kind, gts, fg_masks), dtype=np.uint8)
                    assert s.done(), 'oracle'
                    changed += int(not np.array_equal(want, img))
                    for pname, plan_c, batch in paths:
                        monkeypatch.setattr(oa_mix, 'PLAN_IN_C', plan_c)
                        monkeypatch.setattr(oa_mix, 'BATCH_BOXES', batch)
                        s = C.Script(draws)
                        oa_mix.use_random_state(s)
                        try:
                            T = mix._bboxes_only(st, src, kind, dict(n_tmp=0, luts_for=None))
                        finally:
                            oa_mix.use_random_state(None)
                        assert s.done(), (pname, 'product')
                        got = T.cpu().numpy()
                        bad = int((got != want).sum())
                        assert bad == 0, f'{bname} {kind} level {u_level} sign {u_sign} {pname}: {bad} bytes differ'
                        stats[f'bboxes_only_{kind} {pname}'] += (1, want.size)
    assert np.array_equal(src.cpu().numpy(), img), 'the source image was written'
    if name == 'noise':        # at least: 4 box sets with a live mask x (2 shears x 2 levels + 3 other kinds at the high level) x 2 signs
        assert changed >= 4 * (2 * 2 + 3) * 2, f'only {changed} cases change the image'
    _report(f'bboxes_only on {name} {H} x {W}', stats, t0)


def _norm_args():
    mean = (ctypes.c_float * 3)(*C.MEAN)
    stdinv = (ctypes.c_float * 3)(*[float(np.float32(1.0 / s)) for s in C.STD])
    return mean, stdinv


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def _check_norm(out, u8, to_rgb, what):
    """out [Hp, Wp, 3] fp32 / bf16: inside the image the float32 Normalize of ``u8`` (bf16: that tensor's .bfloat16()), bit
    for bit; every padded element +0.0"""
    import torch
    H, W = u8.shape[:2]
    want = torch.from_numpy(np.ascontiguousarray(C.normalized(u8, to_rgb))).to(out.dtype)
    assert np.array_equal(_bits(out[:H, :W]), _bits(want)), f'{what}: normalised values'
    assert not _bits(out[H:]).any() and not _bits(out[:, W:]).any(), f'{what}: padding'
    return out.numel() * out.element_size()


NORM_VIEWS = (('f32 rgb', 0, 1), ('f32 bgr', 0, 0), ('bf16 rgb', 1, 1))
# the final mix's outputs: (name, normalised dtype or None, to_rgb, with the uint8 view) - the batch pipeline asks for the
# normalised view alone, the dict API for the uint8 view alone
MIX_VIEWS = (('f32 rgb', 0, 1, True), ('f32 bgr', 0, 0, True), ('bf16 rgb', 1, 1, True), ('bf16 rgb alone', 1, 1, False),
             ('u8 alone', None, 0, True))


@gpu
@pytest.mark.parametrize('H,W', C.SIZES_MIX)
def test_final_mix_and_final_tiles_equal_the_oracle(dev, monkeypatch, H, W):
    """section D: m_beta x m_oa rotation x target sets; uint8, fp32 and bf16 views, padded; final == final_tiles == oracle"""
    import torch
    L, lib = _lib(), _lib().lib()
    t0, stats = time.time(), _Stats()
    img, acc = C.mix_inputs(H, W)
    d_img, d_acc = _up(img, dev), _up(acc, dev)
    mean, stdinv = _norm_args()
    Hp, Wp = H + 3, W + 5
    for tname, _ in C.mix_targets(H, W):
        for m_beta in C.M_BETAS:
            for shift in range(3):
                want, masks, m_oas, fg, tlist = _mix_reference(monkeypatch, H, W, tname, m_beta, shift)
                n = len(tlist)
                tg = np.zeros((n,), L.MIX_TARGET)
                fi = 0
                for t, (kind, box) in enumerate(tlist):
                    if kind == 'fg':
                        tg[t] = (fi, (0, 0, 0, 0), m_oas[t])
                        fi += 1
                    else:
                        tg[t] = (-1, tuple(box), m_oas[t])
                d_tg = _up(tg.view(np.uint8).reshape(-1), dev) if n else None
                My = Mx = None
                rects = np.zeros((max(len(fg), 1), 4), np.int32)
                if fg:
                    prof = [cv.box_mask_profiles(np.array(b, np.float32), H, W, 4, 0.3) for b in fg]
                    My, Mx = _up(np.stack([p[0] for p in prof]), dev), _up(np.stack([p[1] for p in prof]), dev)
                    for k, (py, px) in enumerate(prof):        # the tight support of the mask: x0, y0, w, h
                        ys, xs = np.nonzero(py)[0], np.nonzero(px)[0]
                        rects[k] = (xs[0], ys[0], xs[-1] - xs[0] + 1, ys[-1] - ys[0] + 1)
                d_rects = _up(rects, dev)
                nb = int(lib.oadg_oamix_final_tiles_workspace_bytes(H, W, n))
                ws = torch.empty((max(nb, 16),), dtype=torch.uint8, device=dev)
                for form in ('final', 'final_tiles'):
                    if form == 'final_tiles' and n == 0:
                        continue
                    for vname, dt, to_rgb, with_u8 in MIX_VIEWS:
                        u8 = torch.full((H, W, 3), 0xA5, dtype=torch.uint8, device=dev) if with_u8 else None
                        norm, hp, wp = None, H, W
                        if dt is not None:
                            norm, hp, wp = torch.full((Hp, Wp, 3), float('nan'), dtype=torch.bfloat16 if dt else torch.float32,
                                                      device=dev), Hp, Wp
                        nrm = (mean, stdinv) if norm is not None else (None, None)
                        if form == 'final':
                            L.check(lib.oadg_oamix_final(_ptr(d_img), _ptr(d_acc), H, W, _ptr(d_tg), n, _ptr(My), _ptr(Mx),
                                                         float(m_beta), *nrm, to_rgb, _ptr(u8), _ptr(norm), dt or 0, hp, wp,
                                                         L.stream_ptr()), 'oadg_oamix_final')
                        else:
                            L.check(lib.oadg_oamix_final_tiles(_ptr(d_img), _ptr(d_acc), H, W, _ptr(d_tg), n, _ptr(d_rects),
                                                               _ptr(My), _ptr(Mx), float(m_beta), *nrm, to_rgb, _ptr(u8),
                                                               _ptr(norm), dt or 0, hp, wp, _ptr(ws), nb, L.stream_ptr()),
                                    'oadg_oamix_final_tiles')
                        LEDGER['finals'][form] += 1
                        what = f'{form} {tname} m_beta {m_beta} shift {shift} {vname}'
                        nbytes = 0
                        if with_u8:
                            got = u8.cpu().numpy()
                            bad = int((got != want).sum())
                            assert bad == 0, f'{what}: {bad} bytes differ from the oracle'
                            nbytes += got.size
                        if norm is not None:
                            nbytes += _check_norm(norm, want, to_rgb, what)
                        stats[f'{form} {vname}'] += (1, nbytes)
    _report(f'final mix {H} x {W}', stats, t0)


@gpu
@pytest.mark.parametrize('H,W', C.SIZES_MIX)
def test_normalize(dev, H, W):
    """oadg_oamix_normalize on the images of D and of A, padded and not"""
    import torch
    L, lib = _lib(), _lib().lib()
    t0, stats = time.time(), _Stats()
    mean, stdinv = _norm_args()
    for img in [C.mix_inputs(H, W)[0]] + [C.image(n, H, W) for n in C.IMAGES]:
        d_img = _up(img, dev)
        for Hp, Wp in ((H, W), (H + 3, W + 5), (H, W + 1), (H + 1, W)):
            for vname, dt, to_rgb in NORM_VIEWS:
                out = torch.full((Hp, Wp, 3), float('nan'), dtype=torch.bfloat16 if dt else torch.float32, device=dev)
                L.check(lib.oadg_oamix_normalize(_ptr(d_img), H, W, mean, stdinv, to_rgb, _ptr(out), dt, Hp, Wp,
                                                 L.stream_ptr()), 'oadg_oamix_normalize')
                stats[f'normalize {vname}'] += (1, _check_norm(out, img, to_rgb, f'normalize {vname} pad {Hp} x {Wp}'))
    _report(f'normalize {H} x {W}', stats, t0)


@gpu
def test_every_op_kind_and_kernel_form_was_launched(dev):
    """the ledger of this module's GPU tests (run the module as a whole): all 12 OADG_OP_* kinds, both compose kernels, both
    final-mix forms"""
    print('op kinds launched:', dict(sorted(LEDGER['kinds'].items())))
    print('compose kernels:', dict(LEDGER['kernels']), ' final mix:', dict(LEDGER['finals']))
    assert sorted(k for k, v in LEDGER['kinds'].items() if v > 0) == list(range(12)), 'run the whole module'
    assert LEDGER['kernels']['compose_kernel'] > 0 and LEDGER['kernels']['compose4_kernel'] > 0
    assert LEDGER['finals']['final'] > 0 and LEDGER['finals']['final_tiles'] > 0
