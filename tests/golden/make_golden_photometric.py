"""Generate tests/golden/photometric_reference.npz: the GENUINE reference ``PhotoMetricDistortion`` and ``CutOut``
(mmdet/datasets/pipelines/transforms.py:941-1041, :1874-1944) on fixed inputs.  mmcv and cv2 are absent, so
``mmcv.bgr2hsv`` / ``mmcv.hsv2bgr`` resolve to the numpy float32 stand-ins below: OpenCV's documented float32 HSV algorithm
with H in 0..360, one correctly rounded float32 operation per step.  The fixture pins what the reference owns - the random
draws and their order, the order of the sub-steps, the in-place float32 arithmetic around the colour conversion, the hole
arithmetic and the fill - and this restatement of the conversion; cv2's own last-bit rounding stays "parity unpinned".

Inputs: A 37 x 53 (every (b, g, r) of {0, 1, 2, 127, 128, 254, 255}^3, then a hue ramp through 0 / 360 degrees, then noise),
ONE 1 x 1, B 32 x 64 (a ramp round the hue circle, then noise).  PhotoMetricDistortion: seeds 0..15 through np.random.seed
(image seed % 3) and, on the first 10 rows of A (the triples and the ramp), every on / off combination of the five sub-steps
in both modes, forced through a stub random state that returns scripted values.  CutOut: ``CUTOUT_CASES``.
Run here only:  python tests/golden/make_golden_photometric.py
"""
import colorsys
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import refload  # noqa: E402

F = np.float32
EPS = F(np.finfo(np.float32).eps)
LEVELS = (0, 1, 2, 127, 128, 254, 255)
FORCED_ROWS = 10
# flag word of a case (the values of OADG_PHOTO_* in include/oadg_hip.h)
PRESENT, DELTA, ALPHA_PRE, SAT, HUE, ALPHA_POST, PERM = 1, 2, 4, 8, 16, 32, 64

CUTOUT_CASES = [   # (tag, image, seed, CutOut kwargs); image 'F' = the float32 output of PhotoMetricDistortion seed 0 (on A)
    ('ratio', 'A', 0, dict(n_holes=(1, 5), cutout_ratio=(0.2, 0.3), fill_in=(10, 200, 30))),
    ('shape', 'B', 1, dict(n_holes=3, cutout_shape=(8, 5))),
    ('shape_list', 'A', 2, dict(n_holes=(2, 6), cutout_shape=[(4, 4), (10, 3), (1, 9)], fill_in=(255, 0, 7))),
    ('ratio_list', 'B', 3, dict(n_holes=(1, 4), cutout_ratio=[(0.1, 0.1), (0.5, 0.25)])),
    ('none', 'A', 4, dict(n_holes=0, cutout_shape=(4, 4))),
    ('single', 'B', 5, dict(n_holes=1, cutout_shape=(40, 20), fill_in=(1, 2, 3))),
    ('seventy', 'B', 6, dict(n_holes=70, cutout_shape=[(3, 3), (5, 2)], fill_in=(9, 9, 9))),    # overlapping, last row / column
    ('pixel', 'ONE', 7, dict(n_holes=2, cutout_shape=(4, 4), fill_in=(5, 6, 7))),           # starts in the last row and column
    ('zero', 'A', 8, dict(n_holes=(2, 4), cutout_ratio=(0.01, 0.5), fill_in=(50, 60, 70))),     # int(0.01 * 53) = 0: empty
    ('trunc', 'B', 9, dict(n_holes=(1, 5), cutout_ratio=(0.3, 0.3), fill_in=(12.7, 99.9, 0.5))),  # uint8 image: 12, 99, 0
    ('float_fill', 'F', 10, dict(n_holes=(1, 5), cutout_ratio=(0.3, 0.3), fill_in=(12.5, 0.25, 250.75))),
]


# ------------------------------------------------------------------------------------------------- mmcv stand-ins
def bgr2hsv(img):
    """cv2.cvtColor(img, COLOR_BGR2HSV) for float32: H in 0..360, S = diff / (|V| + eps), nothing clamped"""
    assert img.dtype == np.float32
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    s = diff / (np.abs(v) + EPS)
    d = F(60) / (diff + EPS)
    h = np.where(v == r, (g - b) * d, np.where(v == g, (b - r) * d + F(120), (r - g) * d + F(240)))
    h = np.where(h < 0, h + F(360), h)
    return np.stack([h, s, v], axis=-1).astype(np.float32)


SECTOR_TAB = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def hsv2bgr(img):
    """cv2.cvtColor(img, COLOR_HSV2BGR) for float32, H in 0..360"""
    assert img.dtype == np.float32
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    h6 = h * F(6 / 360)
    h6 = np.where(h6 < 0, h6 + F(6), np.where(h6 >= 6, h6 - F(6), h6))
    fl = np.floor(h6)
    f = h6 - fl
    sector = fl.astype(np.int64)
    bad = (sector < 0) | (sector > 5)
    sector = np.where(bad, 0, sector)
    f = np.where(bad, F(0), f)
    one = F(1)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], axis=-1)
    out = np.take_along_axis(tab, SECTOR_TAB[sector], axis=-1)
    out = np.where((s == 0)[..., None], v[..., None], out)
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------- inputs
def _hue_pixels(degrees, s=0.8, v=200.0):
    out = []
    for dg in degrees:
        r, g, b = colorsys.hsv_to_rgb((dg % 360.0) / 360.0, s, 1.0)
        out.append([round(b * v), round(g * v), round(r * v)])
    return np.array(out, dtype=np.uint8)


def images():
    rs = np.random.RandomState(4242)
    triples = np.array([[b, g, r] for b in LEVELS for g in LEVELS for r in LEVELS], dtype=np.uint8)
    ramp = _hue_pixels(np.arange(-26.5, 26.5, 0.5))                     # 106 pixels through 0 / 360 degrees
    n = 37 * 53
    a = np.concatenate([triples, ramp, rs.randint(0, 256, (n - len(triples) - len(ramp), 3)).astype(np.uint8)])
    assert len(triples) + len(ramp) <= FORCED_ROWS * 53
    circle = _hue_pixels(np.arange(0, 360, 360 / 128), s=0.6, v=255.0)
    b = np.concatenate([circle, rs.randint(0, 256, (32 * 64 - len(circle), 3)).astype(np.uint8)])
    return dict(A=a.reshape(37, 53, 3), ONE=np.array([[[17, 200, 93]]], dtype=np.uint8), B=b.reshape(32, 64, 3))


# ------------------------------------------------------------------------------------------------- draw recorders
class Recorder:
    """stands where the reference module's ``random`` (numpy.random) is: delegates and keeps (name, value) of every call"""

    def __init__(self, target):
        self.target, self.calls = target, []

    def __getattr__(self, name):
        fn = getattr(self.target, name)

        def call(*a, **k):
            v = fn(*a, **k)
            self.calls.append((name, v))
            return v
        return call


class Scripted:
    """a stub random state: ``randint`` returns the scripted on / off values in call order, ``uniform`` / ``permutation``
    draw from a private RandomState (inside the requested range)"""

    def __init__(self, ints, seed):
        self.ints, self.rs = list(ints), np.random.RandomState(seed)

    def randint(self, *a):
        return self.ints.pop(0)

    def uniform(self, lo, hi):
        return self.rs.uniform(lo, hi)

    def permutation(self, n):
        return self.rs.permutation(n)


def photo_params(calls):
    """the (name, value) record of one PhotoMetricDistortion call -> (float32 [5] delta, alpha_pre, sat, hue, alpha_post;
    int32 [5] flags, mode, perm)"""
    it = iter(calls)

    def nxt(name):
        n, v = next(it)
        assert n == name, (n, name)
        return v
    flags, vals, perm = PRESENT, [F(0), F(1), F(1), F(0), F(1)], [0, 1, 2]

    def maybe(slot, bit):
        nonlocal flags
        if nxt('randint'):
            vals[slot] = F(nxt('uniform'))
            flags |= bit
    maybe(0, DELTA)
    mode = int(nxt('randint'))
    if mode == 1:
        maybe(1, ALPHA_PRE)
    maybe(2, SAT)
    maybe(3, HUE)
    if mode == 0:
        maybe(4, ALPHA_POST)
    if nxt('randint'):
        perm = [int(v) for v in nxt('permutation')]
        flags |= PERM
    assert next(it, None) is None
    return np.array(vals, dtype=np.float32), np.array([flags, mode] + perm, dtype=np.int32)


class NumpyProxy:
    """stands where the reference module's ``np`` is while CutOut runs: records np.random.randint and np.clip"""

    def __init__(self):
        self.random, self.clips = Recorder(np.random), []

    def clip(self, *a, **k):
        v = np.clip(*a, **k)
        self.clips.append(int(v))
        return v

    def __getattr__(self, name):
        return getattr(np, name)


def main():
    refload.install()
    mm = sys.modules['mmcv']
    mm.bgr2hsv, mm.hsv2bgr = bgr2hsv, hsv2bgr
    T = refload.ref('mmdet.datasets.pipelines.transforms')
    imgs = images()
    out = {k: v for k, v in imgs.items()}
    names = ['A', 'ONE', 'B']
    keep_random, keep_np = T.random, T.np

    def run_photo(tag, img, rnd):
        T.random = rnd
        try:
            res = T.PhotoMetricDistortion()(dict(img=img.copy(), img_fields=['img']))
        finally:
            T.random = keep_random
        assert res['img'].dtype == np.float32
        out[tag + '_out'] = np.ascontiguousarray(res['img'])
        return res['img']

    lo, hi = 0.0, 0.0
    for seed in range(16):
        tag = f'seed{seed}'
        np.random.seed(seed)
        rec = Recorder(np.random)
        o = run_photo(tag, imgs[names[seed % 3]], rec)
        out[tag + '_rng_after'] = np.array([np.random.uniform()])
        out[tag + '_params'], out[tag + '_ints'] = photo_params(rec.calls)
        lo, hi = min(lo, float(o.min())), max(hi, float(o.max()))
    head = imgs['A'][:FORCED_ROWS]
    for mode in (0, 1):
        for bits in range(32):
            on = [(bits >> k) & 1 for k in range(5)]                    # brightness, contrast, saturation, hue, swap
            ints = [on[0], mode] + ([on[1], on[2], on[3]] if mode == 1 else [on[2], on[3], on[1]]) + [on[4]]
            stub = Scripted(ints, 1000 + 32 * mode + bits)
            rec = Recorder(stub)
            tag = f'forced_m{mode}_{bits:02d}'
            o = run_photo(tag, head, rec)
            assert not stub.ints
            out[tag + '_params'], out[tag + '_ints'] = photo_params(rec.calls)
            lo, hi = min(lo, float(o.min())), max(hi, float(o.max()))
    print('PhotoMetricDistortion outputs range from %.1f to %.1f (nothing is clamped)' % (lo, hi))

    imgs['F'] = out['seed0_out']
    for tag, name, seed, kw in CUTOUT_CASES:
        proxy = NumpyProxy()
        np.random.seed(100 + seed)
        T.np = proxy
        try:
            res = T.CutOut(**kw)(dict(img=imgs[name].copy()))
        finally:
            T.np = keep_np
        draws = [v for n, v in proxy.random.calls]
        assert all(n == 'randint' for n, _ in proxy.random.calls) and (len(draws) - 1) % 3 == 0
        n = int(draws[0])
        assert len(draws) == 1 + 3 * n and len(proxy.clips) == 2 * n
        rects = np.array([[draws[1 + 3 * i], draws[2 + 3 * i], proxy.clips[2 * i], proxy.clips[2 * i + 1]] for i in range(n)],
                         dtype=np.int32).reshape(n, 4)
        h, w = imgs[name].shape[:2]
        if tag in ('seventy', 'pixel'):
            assert (rects[:, 0] == w - 1).any() and (rects[:, 1] == h - 1).any(), tag
        if tag == 'zero':
            assert n and (rects[:, 2] == rects[:, 0]).all()
        assert res['img'].dtype == imgs[name].dtype
        out[f'cutout_{tag}_out'] = np.ascontiguousarray(res['img'])
        out[f'cutout_{tag}_rects'] = rects
        out[f'cutout_{tag}_rng_after'] = np.array([np.random.uniform()])
    out['cutout_cases'] = np.array([repr(CUTOUT_CASES)])               # read back with ast.literal_eval (tuples stay tuples)
    # how far the float32 round trip through the stand-ins is from the identity on random bytes
    x = np.random.RandomState(7).randint(0, 256, (256, 256, 3)).astype(np.float32)
    print('HSV round trip on random bytes: at most %.2g grey levels off' % float(np.abs(hsv2bgr(bgr2hsv(x)) - x).max()))
    path = os.path.join(HERE, 'photometric_reference.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
