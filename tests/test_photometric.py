"""PhotoMetricDistortion / CutOut (oadg_amd.pipelines.photometric) against tests/golden/photometric_reference.npz, which the
GENUINE reference classes wrote (tests/golden/make_golden_photometric.py): the draws and their order to the float32 bit, the
rectangles, the generator's state afterwards - and a numpy restatement of the per-pixel chain of csrc/photo.hip
(``photo_chain`` / ``restate`` below) that reproduces every fixture output bit for bit.  That restatement is what
tests/test_hip_photo.py holds the kernel against; here it also guards the fixture.  The float32 HSV conversion is OpenCV's
documented algorithm restated in numpy; cv2's own last-bit rounding is not pinned (neither cv2 nor mmcv is available).
No GPU is needed: DevicePipeline's constructor and the configs are checked as far as the host goes."""
import ast
import os

import numpy as np
import pytest

F = np.float32
EPS = F(np.finfo(np.float32).eps)
PRESENT, DELTA, ALPHA_PRE, SAT, HUE, ALPHA_POST, PERM, CUTOUT_LAST = 1, 2, 4, 8, 16, 32, 64, 128
IMAGES = ('A', 'ONE', 'B')
FORCED_ROWS = 10
SEEDED = [f'seed{s}' for s in range(16)]
FORCED = [f'forced_m{m}_{b:02d}' for m in (0, 1) for b in range(32)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'photometric_reference.npz'))


def cutout_cases(g):
    return ast.literal_eval(str(g['cutout_cases'][0]))


def case_image(g, tag):
    """the uint8 input of a PhotoMetricDistortion case"""
    return g['A'][:FORCED_ROWS] if tag.startswith('forced') else g[IMAGES[int(tag[4:]) % 3]]


def case_params(g, tag):
    """a fixture case as the record PhotoMetricDistortion.draw() returns"""
    v, i = g[tag + '_params'], g[tag + '_ints']
    return dict(flags=int(i[0]), mode=int(i[1]), delta=v[0], alpha_pre=v[1], sat=v[2], hue=v[3], alpha_post=v[4],
                perm=tuple(int(k) for k in i[2:5]))


# ------------------------------------------------------------------------------------ the kernel's per-pixel chain in numpy
B_TAB, G_TAB, R_TAB = (1, 1, 3, 0, 0, 2), (3, 0, 0, 2, 1, 1), (0, 2, 1, 1, 3, 0)     # tab index of b, g, r per sector


def photo_chain(x, p):
    """csrc/photo.hip photo_chain on a float32 [..., 3] BGR array: one float32 operation per step, branches as masks"""
    x = np.array(x, dtype=np.float32)
    fl = int(p['flags'])
    if fl & DELTA:
        x = x + F(p['delta'])
    if fl & ALPHA_PRE:
        x = x * F(p['alpha_pre'])
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v, vmin = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    s = diff / (np.abs(v) + EPS)
    d = F(60) / (diff + EPS)
    is_r = v == r
    is_g = ~is_r & (v == g)
    h = (r - g) * d + F(240)
    h[is_g] = ((b - r) * d + F(120))[is_g]
    h[is_r] = ((g - b) * d)[is_r]
    h[h < 0] += F(360)
    if fl & SAT:
        s = s * F(p['sat'])
    if fl & HUE:
        h = h + F(p['hue'])
        h[h > 360] -= F(360)
        h[h < 0] += F(360)
    h6 = h * F(6 / 360)
    low = h6 < 0
    high = ~low & (h6 >= 6)
    h6[low] += F(6)
    h6[high] -= F(6)
    floor = np.floor(h6)
    f = h6 - floor
    sector = floor.astype(np.int64)
    outside = (sector < 0) | (sector > 5)
    sector[outside], f[outside] = 0, 0
    one = F(1)
    tab = [v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))]
    grey = s == 0
    out = np.stack([np.where(grey, v, np.choose(np.take(t, sector), tab)) for t in (B_TAB, G_TAB, R_TAB)], axis=-1)
    if fl & ALPHA_POST:
        out = out * F(p['alpha_post'])
    if fl & PERM:
        out = out[..., list(p['perm'])]
    assert out.dtype == np.float32
    return out


def cut(x, rects, fill):
    """the holes of ``rects`` (int32 [n, 4] = x1, y1, x2, y2, exclusive) filled in a copy of ``x``"""
    x = x.copy()
    for x1, y1, x2, y2 in np.asarray(rects).reshape(-1, 4):
        x[y1:y2, x1:x2] = np.asarray(fill).astype(x.dtype)
    return x


def normalize(x, mean, stdinv, to_rgb, Hp, Wp):
    """mmcv.imnormalize + Pad on a float32 [H, W, 3] image -> float32 [Hp, Wp, 3]"""
    x = x[..., ::-1] if to_rgb else x
    out = np.zeros((Hp, Wp, 3), np.float32)
    out[:x.shape[0], :x.shape[1]] = (x.astype(np.float32) - np.asarray(mean, np.float32)) * np.asarray(stdinv, np.float32)
    return out


def restate(img_u8, photo, rects, fill, cutout_last, mean, stdinv, to_rgb, Hp, Wp):
    """what oadg_photo_normalize_batch writes for one image (include/oadg_hip.h), in numpy float32"""
    x = img_u8.astype(np.float32)
    fill = np.asarray(fill, np.float32)
    if not cutout_last:
        x = cut(x, rects, fill)
    if photo is not None:
        x = photo_chain(x, photo)
    if cutout_last:
        x = cut(x, rects, fill)
    return normalize(x, mean, stdinv, to_rgb, Hp, Wp)


def norm_args():
    from oadg_amd.pipelines import Normalize
    a = Normalize(MEAN, STD).as_args()
    return a['mean'], a['stdinv']


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Scripted:
    """the generator's stub random state: scripted on / off draws, values from a private RandomState"""

    def __init__(self, ints, seed):
        self.ints, self.rs = list(ints), np.random.RandomState(seed)

    def randint(self, *a):
        return self.ints.pop(0)

    def uniform(self, lo, hi):
        return self.rs.uniform(lo, hi)

    def permutation(self, n):
        return self.rs.permutation(n)


def forced_stub(tag):
    mode, b = int(tag[8]), int(tag[10:])
    on = [(b >> k) & 1 for k in range(5)]                    # brightness, contrast, saturation, hue, swap
    ints = [on[0], mode] + ([on[1], on[2], on[3]] if mode == 1 else [on[2], on[3], on[1]]) + [on[4]]
    return Scripted(ints, 1000 + 32 * mode + b)


def same_params(p, q):
    return all(bits(p[k]).tolist() == bits(q[k]).tolist() for k in ('delta', 'alpha_pre', 'sat', 'hue', 'alpha_post')) and \
        (p['flags'], p['mode'], tuple(p['perm'])) == (q['flags'], q['mode'], tuple(q['perm']))


# ------------------------------------------------------------------------------------------------------------- registry
PHOTO_CFG = dict(type='PhotoMetricDistortion')
CUTOUT_CFG = dict(type='CutOut', n_holes=(1, 5), cutout_ratio=[(0.1, 0.2), (0.25, 0.1)])
HEAD = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
        dict(type='Resize', img_scale=[(128, 50), (128, 64)], keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5)]
TAIL = [dict(type='Normalize', mean=MEAN, std=STD, to_rgb=True), dict(type='Pad', size_divisor=32),
        dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def test_both_types_build_from_the_registry():
    from oadg_amd.pipelines import Compose
    from oadg_amd.pipelines.photometric import CutOut, PhotoMetricDistortion
    p, c = Compose([dict(type='PhotoMetricDistortion', brightness_delta=16, hue_delta=9), CUTOUT_CFG]).transforms
    assert isinstance(p, PhotoMetricDistortion) and (p.brightness_delta, p.hue_delta, p.contrast_upper) == (16, 9, 1.5)
    assert isinstance(c, CutOut) and c.n_holes == (1, 5) and c.with_ratio and len(c.candidates) == 2


def test_cutout_constructor_asserts_what_the_reference_asserts():
    from oadg_amd.pipelines.photometric import CutOut
    for kw in (dict(n_holes=1), dict(n_holes=1, cutout_shape=(2, 2), cutout_ratio=(0.1, 0.1)), dict(n_holes=(3, 3), cutout_shape=(2, 2)),
               dict(n_holes=(1, 2, 3), cutout_shape=(2, 2)), dict(n_holes=(-1, 2), cutout_shape=(2, 2))):
        with pytest.raises(AssertionError):
            CutOut(**kw)
    for fill in ((0, 0, 256), (-1, 0, 0), (0, float('nan'), 0)):
        with pytest.raises(ValueError, match='fill_in'):
            CutOut(n_holes=1, cutout_shape=(2, 2), fill_in=fill)
    c = CutOut(n_holes=2, cutout_shape=(2, 2), fill_in=(12.7, 99.9, 0.5))
    assert c.n_holes == (2, 2) and c.candidates == [(2, 2)]
    assert c.fill(on_uint8=True).tolist() == [12, 99, 0] and c.fill(on_uint8=True).dtype == np.float32
    assert bits(c.fill(on_uint8=False)).tolist() == bits(np.array([12.7, 99.9, 0.5], np.float32)).tolist()


# ---------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize('tag', SEEDED)
def test_photo_draw_matches_the_reference_seeded(g, tag):
    from oadg_amd.pipelines.photometric import PhotoMetricDistortion
    np.random.seed(int(tag[4:]))
    p = PhotoMetricDistortion().draw()
    assert same_params(p, case_params(g, tag)), (p, case_params(g, tag))
    assert all(isinstance(p[k], np.float32) for k in ('delta', 'alpha_pre', 'sat', 'hue', 'alpha_post'))
    assert np.random.uniform() == float(g[tag + '_rng_after'][0])


def test_photo_draw_matches_the_reference_in_every_combination(g):
    from oadg_amd.pipelines.oa_mix import use_random_state
    from oadg_amd.pipelines.photometric import PhotoMetricDistortion
    seen = set()
    try:
        for tag in FORCED:
            stub = forced_stub(tag)
            use_random_state(stub)
            p = PhotoMetricDistortion().draw()
            assert not stub.ints and same_params(p, case_params(g, tag)), tag
            seen.add((p['mode'], p['flags']))
    finally:
        use_random_state(None)
    assert len(seen) == 64                                              # 2 modes x 2^5 sub-step combinations, all distinct


def test_cutout_draw_matches_the_reference(g):
    from oadg_amd.pipelines.photometric import CutOut
    cases = cutout_cases(g)
    assert len(cases) == 11
    for tag, name, seed, kw in cases:
        h, w = (g['seed0_out'] if name == 'F' else g[name]).shape[:2]
        np.random.seed(100 + seed)
        rects = CutOut(**kw).draw(h, w)
        want = g[f'cutout_{tag}_rects']
        assert rects.dtype == np.int32 and rects.shape == want.shape and np.array_equal(rects, want), tag
        assert np.random.uniform() == float(g[f'cutout_{tag}_rng_after'][0]), tag
    n = {tag: len(g[f'cutout_{tag}_rects']) for tag, *_ in cases}
    assert n['none'] == 0 and n['single'] == 1 and n['seventy'] == 70
    r = g['cutout_seventy_rects']
    assert (r[:, 0] == 63).any() and (r[:, 1] == 31).any()             # holes that start in the last column / row
    z = g['cutout_zero_rects']
    assert len(z) and (z[:, 0] == z[:, 2]).all()                       # zero-sized holes


# ---------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize('tag', SEEDED + FORCED)
def test_restatement_reproduces_the_reference_output(g, tag):
    want = g[tag + '_out']
    got = photo_chain(case_image(g, tag).astype(np.float32), case_params(g, tag))
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), \
        (tag, int((bits(got) != bits(want)).sum()), float(np.abs(got - want).max()))


def test_fixture_leaves_the_byte_range_and_covers_the_special_pixels(g):
    lo = min(float(g[t + '_out'].min()) for t in SEEDED + FORCED)
    hi = max(float(g[t + '_out'].max()) for t in SEEDED + FORCED)
    assert lo < -50 and hi > 300                                       # nothing is clamped
    head = g['A'][:FORCED_ROWS].reshape(-1, 3).astype(int)
    assert (head.max(1) == head.min(1)).sum() >= 7                      # greys (s == 0), black among them
    assert (head.sum(1) == 0).any() and len({tuple(p) for p in head[:343]}) == 343
    # the ramp: reds on both sides of 0 / 360 degrees (g > b: just above 0, b > g: just below 360), so +-18 wraps both ways
    ramp = head[343:343 + 106]
    assert (ramp[:, 2] == ramp.max(1)).all() and (ramp[:, 1] > ramp[:, 0]).any() and (ramp[:, 0] > ramp[:, 1]).any()


def test_restatement_reproduces_the_reference_cutout(g):
    from oadg_amd.pipelines.photometric import CutOut
    for tag, name, seed, kw in cutout_cases(g):
        img = g['seed0_out'] if name == 'F' else g[name]
        fill = CutOut(**kw).fill(on_uint8=img.dtype == np.uint8)
        got = cut(img, g[f'cutout_{tag}_rects'], fill)
        want = g[f'cutout_{tag}_out']
        assert got.dtype == want.dtype and np.array_equal(got, want), tag
    t = g['cutout_trunc_out'][tuple(g['cutout_trunc_rects'][0][[1, 0]])]
    assert t.tolist() == [12, 99, 0]                                    # a float fill on a uint8 image is truncated


def test_restate_composes_cutout_photometric_and_normalize(g):
    """the float image of the reference's CutOut case 'float_fill' is PhotoMetricDistortion seed 0 followed by CutOut: the
    whole chain of the kernel (CutOut last) against the two genuine steps, then Normalize + Pad by hand"""
    mean, stdinv = norm_args()
    kw = next(c[3] for c in cutout_cases(g) if c[0] == 'float_fill')
    rects = g['cutout_float_fill_rects']
    got = restate(g['A'], case_params(g, 'seed0'), rects, kw['fill_in'], True, mean, stdinv, True, 40, 56)
    want = normalize(g['cutout_float_fill_out'], mean, stdinv, True, 40, 56)
    assert np.array_equal(bits(got), bits(want)) and not got[37:].any() and not got[:, 53:].any()
    first = restate(g['A'], case_params(g, 'seed0'), rects, kw['fill_in'], False, mean, stdinv, True, 40, 56)
    assert len(rects) and not np.array_equal(first, got)


# ------------------------------------------------------------------------------------------------------ DevicePipeline
def test_device_pipeline_accepts_the_new_steps_in_either_order():
    from oadg_amd.pipelines import DevicePipeline
    from oadg_amd.pipelines.photometric import CutOut, PhotoMetricDistortion
    d = DevicePipeline(HEAD + [PHOTO_CFG, CUTOUT_CFG] + TAIL)
    assert [type(t) for t in d.photo_steps] == [PhotoMetricDistortion, CutOut] and d.cutout_last
    d = DevicePipeline(HEAD + [CUTOUT_CFG, PHOTO_CFG] + TAIL)
    assert [type(t) for t in d.photo_steps] == [CutOut, PhotoMetricDistortion] and not d.cutout_last
    d = DevicePipeline([CUTOUT_CFG] + TAIL)
    assert d.photo is None and isinstance(d.cutout, CutOut) and not d.cutout_last
    d = DevicePipeline(HEAD[:2] + [PHOTO_CFG] + TAIL)
    assert isinstance(d.photo, PhotoMetricDistortion) and d.cutout is None
    assert DevicePipeline(HEAD + TAIL).photo_steps == []


OAMIX_CFG = dict(type='OAMix', version='augmix', num_views=2, keep_orig=True, severity=10, random_box_ratio=(3, 1 / 3),
                 random_box_scale=(0.01, 0.1), oa_random_box_scale=(0.005, 0.1), oa_random_box_ratio=(3, 1 / 3),
                 spatial_ratio=4, sigma_ratio=0.3)


def _test_pipeline(inner_extra, outer_extra=()):
    return [dict(type='LoadImageFromFile')] + list(outer_extra) + [
        dict(type='MultiScaleFlipAug', img_scale=(128, 64), flip=False,
             transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip')] + list(inner_extra) + [
                 dict(type='Normalize', mean=MEAN, std=STD, to_rgb=True), dict(type='Pad', size_divisor=32),
                 dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]


@pytest.mark.parametrize('pipeline,names', [
    (HEAD[:2] + [PHOTO_CFG] + HEAD[2:] + TAIL, 'PhotoMetricDistortion in front of Resize'),
    (HEAD[:3] + [CUTOUT_CFG] + HEAD[3:] + TAIL, 'CutOut in front of RandomFlip'),
    (HEAD + TAIL[:1] + [PHOTO_CFG] + TAIL[1:], 'PhotoMetricDistortion behind Normalize'),
    (HEAD + TAIL[:1] + [CUTOUT_CFG] + TAIL[1:], 'CutOut behind Normalize'),
    (_test_pipeline([PHOTO_CFG]), 'PhotoMetricDistortion inside MultiScaleFlipAug'),
    (_test_pipeline([CUTOUT_CFG]), 'CutOut inside MultiScaleFlipAug'),
    (_test_pipeline([], [CUTOUT_CFG]), 'CutOut beside MultiScaleFlipAug'),
    ([OAMIX_CFG, PHOTO_CFG] + TAIL, 'PhotoMetricDistortion together with OAMix'),
    ([CUTOUT_CFG, OAMIX_CFG] + TAIL, 'CutOut together with OAMix'),
    (HEAD + [PHOTO_CFG, CUTOUT_CFG, PHOTO_CFG] + TAIL, 'PhotoMetricDistortion appears more than once'),
    (HEAD + [CUTOUT_CFG, CUTOUT_CFG] + TAIL, 'CutOut appears more than once'),
], ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else None)
def test_device_pipeline_rejects_with_the_name_of_the_step(pipeline, names):
    from oadg_amd.pipelines import DevicePipeline
    with pytest.raises(ValueError, match=names):
        DevicePipeline(pipeline)


@pytest.mark.parametrize('name,step', [('photo', 'PhotoMetricDistortion'), ('cutout', 'CutOut')])
def test_the_new_configs_load_and_their_pipelines_build(name, step):
    from oadg_amd import Config
    from oadg_amd.pipelines import DevicePipeline
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'oadg', f'faster_rcnn_r50_fpn_1x_cityscapes_{name}.py'))
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r50_fpn_1x_cityscapes.py'))
    pipe = cfg.data.train.pipeline
    assert [t['type'] for t in pipe] == [step] + [t['type'] for t in base.data.train.pipeline]
    assert [dict(t) for t in pipe[1:]] == [dict(t) for t in base.data.train.pipeline]
    assert dict(cfg.model) == dict(base.model) and dict(cfg.optimizer) == dict(base.optimizer)
    d = DevicePipeline(pipe)
    assert [type(t).__name__ for t in d.photo_steps] == [step]
    if name == 'cutout':
        assert d.cutout.n_holes == (1, 5) and d.cutout.with_ratio and len(d.cutout.candidates) > 1
    else:
        assert (d.photo.brightness_delta, d.photo.contrast_lower, d.photo.saturation_upper, d.photo.hue_delta) == (32, 0.5, 1.5, 18)


def test_pipelines_never_spell_the_c_symbol():
    """the ctypes call lives in oadg_photo.py, next to the import shim (tests/test_target_audit.py's closure)"""
    import re
    for f in ('photometric.py', 'device_pipeline.py'):
        assert not re.search(r'\.oadg_photo', open(os.path.join(ROOT, 'oa-dg_amd', 'pipelines', f)).read())
    assert 'tests/test_hip_photo.py' in open(os.path.join(ROOT, 'oadg_photo.py')).read()
