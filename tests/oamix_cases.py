"""Case builders and plain references for tests/test_oamix_ops.py: the region ops, the histogram / LUT kernels and the final
mix of csrc/oamix.hip, one op at a time on degenerate images.  CPU only, imports without a GPU.

Images (uint8 [H, W, 3], seeded by name and size, returned read-only and shared):
  noise         uniform 0..255 (0 and 255 present)
  flat          per-channel constants 7, 0, 255
  one_outlier   all 9 except the LAST pixel [200, 9, 250] (with H*W % 4 != 0 it lies in hist_kernel's tail)
  sat_checker   a 0 / 255 checkerboard
  binary_noise  random 0 / 255
  narrow        channel 0 in 100..103, channel 1 flat 50, channel 2 full range
  ramp          channel 0 = 20 + 200 x / (W - 1) (a non-integer autocontrast scale), channel 1 = 255 y / (H - 1),
                channel 2 in {254, 255}

The NumPy restatement below repeats the kernels' colour arithmetic operation for operation (float32 where the kernel is
float32, float64 where it is float64, truncation where it truncates); tests/test_oamix_ops.py holds it to Pillow on every
case before it is used for anything, and plants errors in it (``planted``) to show that the cases notice them:
  eq_step0     equalize goes on with step = 1 where step == 0 asks for the identity table
  ac_round     autocontrast rounds to nearest instead of truncating
  blend_clamp  the clamp of Image.blend is applied for factors inside [0, 1] (where it does nothing) and the plain
               truncating cast outside (where the clamp is needed)
  sharp_border the border pixels are filtered too (edge replicated) instead of copied
  mean_half    the contrast mean lacks its + 0.5
  sol_le       solarize keeps v <= threshold instead of v < threshold
  post_bit     the posterize mask keeps one bit less
  hist_tail    the last npix % 4 pixels are missing from the histogram
  rect_right4  a rectangle's right edge is rounded down to a multiple of 4
  rest_moa     the last target's m_oa instead of m_beta weighs the rest term of the final mix
"""
import functools
import zlib

import numpy as np

f32 = np.float32

IMAGES = ('noise', 'flat', 'one_outlier', 'sat_checker', 'binary_noise', 'narrow', 'ramp')
SIZES_MAIN = ((3, 3), (5, 7), (17, 23), (33, 64), (61, 97))       # H*W % 4 = 1, 3, 3, 0, 1
SIZES_THIN = ((1, 9), (9, 2))                                     # no interior for the two-tap 8-byte row loads
SIZE_MULTI = (131, 253)                                           # 33,143 pixels, % 4 == 3, three histogram workgroups
SIZES_A = SIZES_MAIN + SIZES_THIN + (SIZE_MULTI,)
SIZE_BIG = (1025, 2047)                                           # > 8192 x 256 pixels, W % 4 != 0: compose_kernel's second trip
SIZES_WARP = ((1, 9), (9, 2), (17, 23), (33, 64))
SIZES_BOX = ((33, 64), (61, 97))
SIZES_MIX = ((17, 23), (33, 64), (61, 97))

POSTERIZE_BITS = (0, 1, 2, 3, 4)
SOLARIZE_THRESHOLDS = (1, 2, 128, 255, 256)
FACTORS = (0.1, 0.118, 0.5, 0.999, 1.0, 1.0000001, 1.3, 1.9, 0.1 + 0.18 * 9.99)
ENHANCERS = ('color', 'contrast', 'brightness', 'sharpness')
LUT_OPS = ('autocontrast', 'equalize')
PLANTED = ('eq_step0', 'ac_round', 'blend_clamp', 'sharp_border', 'mean_half', 'sol_le', 'post_bit', 'hist_tail',
           'rect_right4', 'rest_moa')

# level draws as unit doubles u (level = 0.1 + 9.9 u, numpy's uniform(0.1, 10)): the extremes 0.1 and 9.999999, one middle
U_LOW, U_MID, U_HIGH = 0.0, 0.5, 0.9999999
U_PLUS, U_MINUS = 0.25, 0.75                                     # sign draws: > 0.5 flips
GEO_KINDS = ('rotate', 'shear_x', 'shear_y', 'translate_x', 'translate_y')
M_BETAS = (0.0, 0.5, 1.0)
M_OA_UNITS = (0.0, 0.25, 0.99999994)                              # the last one only with a score above the threshold
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


def posterize_mask(bits, planted=()):
    if 'post_bit' in planted:
        bits = bits - 1
    return ~(2 ** (8 - bits) - 1) & 255


def color_ops(big=False):
    """every (name, parameter) of section A; ``copy`` and ``image`` complete the region-op kinds of the compose kernels"""
    if big:
        return [('posterize', 2), ('autocontrast', None), ('solarize', 128)]
    ops = [(n, None) for n in LUT_OPS] + [('posterize', b) for b in POSTERIZE_BITS]
    ops += [('solarize', t) for t in SOLARIZE_THRESHOLDS]
    ops += [(e, f) for e in ENHANCERS for f in FACTORS]
    return ops + [('copy', None), ('image', None)]


# ------------------------------------------------------------------------------------------------------------ images
def _rs(name, H, W):
    return np.random.RandomState(zlib.crc32(f'{name}:{H}x{W}'.encode()) & 0x7fffffff)


@functools.lru_cache(maxsize=None)
def image(name, H, W):
    rs = _rs(name, H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    if name == 'noise':
        img = rs.randint(0, 256, (H, W, 3))
        img.reshape(-1)[:2] = (255, 0)
        img.reshape(-1)[-2:] = (0, 255)
    elif name == 'flat':
        img = np.broadcast_to(np.array([7, 0, 255]), (H, W, 3)).copy()
    elif name == 'one_outlier':
        img = np.full((H, W, 3), 9)
        img[H - 1, W - 1] = (200, 9, 250)
    elif name == 'sat_checker':
        img = np.repeat((((yy + xx) & 1) * 255)[..., None], 3, 2)
    elif name == 'binary_noise':
        img = rs.randint(0, 2, (H, W, 3)) * 255
    elif name == 'narrow':
        c2 = rs.randint(0, 256, (H, W))
        c2.reshape(-1)[0], c2.reshape(-1)[-1] = 0, 255
        img = np.stack([100 + rs.randint(0, 4, (H, W)), np.full((H, W), 50), c2], 2)
    elif name == 'ramp':
        img = np.stack([20 + (xx * 200) // max(W - 1, 1), (yy * 255) // max(H - 1, 1), 254 + ((xx + yy) & 1)], 2)
    else:
        raise KeyError(name)
    img = np.ascontiguousarray(img.astype(np.uint8))
    img.setflags(write=False)
    return img


def other_image(img):
    """the second image an OADG_OP_IMAGE region reads"""
    return np.ascontiguousarray(img[::-1, ::-1] ^ np.uint8(0x5A))


# ------------------------------------------------------------------------------------------------------------ Pillow side
def pillow_op(name, param, img):
    """the reference of section A: the op through Pillow on Image.fromarray(img), as oracle.oamix.color_op applies it"""
    from PIL import Image, ImageEnhance, ImageOps
    if name == 'copy':
        return img
    if name == 'image':
        return other_image(img)
    pil = Image.fromarray(img)
    if name == 'autocontrast':
        out = ImageOps.autocontrast(pil)
    elif name == 'equalize':
        out = ImageOps.equalize(pil)
    elif name == 'posterize':
        out = ImageOps.posterize(pil, param)
    elif name == 'solarize':
        out = ImageOps.solarize(pil, param)
    else:
        out = {'color': ImageEnhance.Color, 'contrast': ImageEnhance.Contrast, 'brightness': ImageEnhance.Brightness,
               'sharpness': ImageEnhance.Sharpness}[name](pil).enhance(param)
    return np.asarray(out)


def pillow_gray_sum(img):
    from PIL import Image
    return int(np.asarray(Image.fromarray(img).convert('L')).astype(np.int64).sum())


def lut_from_outputs(img, out):
    """(table [3, 256], present [3, 256] bool): the value -> value map an image and its LUT-op result show"""
    table = np.zeros((3, 256), np.uint8)
    present = np.zeros((3, 256), bool)
    for c in range(3):
        table[c][img[..., c].reshape(-1)] = out[..., c].reshape(-1)
        present[c][img[..., c].reshape(-1)] = True
    return table, present


# ------------------------------------------------------------------------------------------------------------ restatement
def hist3(img, planted=()):
    """hist_kernel: [3, 256] counts"""
    flat = img.reshape(-1, 3)
    if 'hist_tail' in planted:
        flat = flat[:len(flat) // 4 * 4]
    return np.stack([np.bincount(flat[:, c], minlength=256) for c in range(3)]).astype(np.int64)


def equalize_step(h):
    """ImageOps.equalize's step of one channel histogram, None where fewer than two bins are filled"""
    histo = h[h > 0]
    if len(histo) <= 1:
        return None
    return int((histo.sum() - histo[-1]) // 255)


def autocontrast_lut(h, planted=()):
    ident = np.arange(256)
    nz = np.nonzero(h)[0]
    if len(nz) == 0 or nz[-1] <= nz[0]:
        return ident.astype(np.uint8)
    lo, hi = int(nz[0]), int(nz[-1])
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    v = ident.astype(np.float64) * scale + offset
    q = np.rint(v) if 'ac_round' in planted else np.trunc(v)
    return np.clip(q, 0, 255).astype(np.uint8)


def equalize_lut(h, planted=()):
    ident = np.arange(256).astype(np.uint8)
    step = equalize_step(h)
    if step is None:
        return ident
    if step == 0:
        if 'eq_step0' not in planted:
            return ident
        step = 1
    pre = np.cumsum(h) - h
    return np.minimum((step // 2 + pre) // step, 255).astype(np.uint8)


def luts(img, planted=()):
    """luts_kernel on hist_kernel's counts: [2, 3, 256], [0] autocontrast, [1] equalize"""
    h = hist3(img, planted)
    return np.stack([np.stack([autocontrast_lut(h[c], planted) for c in range(3)]),
                     np.stack([equalize_lut(h[c], planted) for c in range(3)])])


def luma(img):
    i = img.astype(np.int64)
    return (i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16


def gray_sum(img):
    return int(luma(img).sum())


def contrast_mean(img, planted=()):
    H, W = img.shape[:2]
    return int(float(gray_sum(img)) / float(H * W) + (0.0 if 'mean_half' in planted else 0.5))


def smooth(img, planted=()):
    """ImageFilter.SMOOTH (3 x 3, 1 1 1 / 1 5 1 / 1 1 1 over 13) in Filter.c's order: float32, rows y+1, y, y-1 added to the
    0.5 offset one after the other, border pixels copied.  Returns (result, interior pixels at the upper clamp)."""
    H, W = img.shape[:2]
    border = 'sharp_border' in planted
    src = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode='edge') if border else img
    out = img.copy()
    h, w = src.shape[:2]
    if h < 3 or w < 3:
        return out, 0
    f = src.astype(f32)
    k1, k5 = f32(1.0) / f32(13.0), f32(5.0) / f32(13.0)
    ss = np.full((h - 2, w - 2, img.shape[2]), 0.5, f32)
    for dy in (1, 0, -1):
        r = f[1 + dy:h - 1 + dy]
        kc = k5 if dy == 0 else k1
        ss = ss + ((r[:, :-2] * k1 + r[:, 1:-1] * kc) + r[:, 2:] * k1)
    q = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.trunc(ss))).astype(np.uint8)
    if border:
        out = q
    else:
        out[1:-1, 1:-1] = q
    return out, int((ss >= 255).sum())


def blend(deg, img, factor, planted=()):
    """Image.blend(degenerate, image, factor): float32; inside [0, 1] a truncating cast, outside clamp then cast.
    Returns (result, values the clamp changed)."""
    alpha = f32(factor)
    a, b = deg.astype(np.int32), img.astype(np.int32)
    t = a.astype(f32) + alpha * (b - a).astype(f32)
    clamp = not (f32(0) <= alpha <= f32(1))
    if 'blend_clamp' in planted:
        clamp = not clamp
    clipped = int(((t <= 0) | (t >= 255)).sum()) if clamp else 0
    if clamp:
        t = np.where(t <= 0, f32(0), np.where(t >= 255, f32(255), t))
    return np.trunc(t).astype(np.int64).astype(np.uint8), clipped


def degenerate(name, img, planted=()):
    if name == 'brightness':
        return np.zeros_like(img)
    if name == 'color':
        return np.repeat(luma(img)[..., None], 3, 2).astype(np.uint8)
    if name == 'contrast':
        return np.full_like(img, contrast_mean(img, planted))
    return smooth(img, planted)[0]


def restated_op(name, param, img, planted=()):
    """one region op of apply_region_op over the whole image"""
    if name == 'copy':
        return img
    if name == 'image':
        return other_image(img)
    if name in LUT_OPS:
        t = luts(img, planted)[LUT_OPS.index(name)]
        return np.stack([t[c][img[..., c]] for c in range(3)], 2)
    if name == 'posterize':
        return img & np.uint8(posterize_mask(param, planted))
    if name == 'solarize':
        v = img.astype(np.int32)
        keep = v <= param if 'sol_le' in planted else v < param
        return np.where(keep, v, 255 - v).astype(np.uint8)
    return blend(degenerate(name, img, planted), img, param, planted)[0]


# ------------------------------------------------------------------------------------------------------------ layouts
def layouts(H, W):
    """rectangle layouts of one compose launch, [(name, [x1, y1, x2, y2] ...)], at most two rectangles, disjoint.  Edges
    that are no multiple of 4 put a region boundary inside one thread's four pixels where W % 4 == 0."""
    a = max(W - 3, 0)                       # left edge of the right-hand rects: 61 at W = 64
    b = min(5, a)                           # right edge of the left-hand rects
    hy = (H + 1) // 2
    return [
        ('none', []),
        ('pixel_top_left', [[0, 0, 1, 1]]),
        ('whole', [[0, 0, W, H]]),
        ('bottom_right', [[a, H // 2, W, H]]),
        ('top_right+bottom_left', [[a, 0, W, hy], [0, hy, b, H]]),
        ('pixel_bottom_right+inner', [[W - 1, H - 1, W, H], [1, 0, max(W - 2, 1), max(H - 1, 0)]]),
    ]


def compose(outs, rects, planted=()):
    """compose_kernel's region selection: outs[k] inside rects[k] (the later rectangle wins), outs[2] outside"""
    res = np.array(outs[2], copy=True)
    for k, (x1, y1, x2, y2) in enumerate(rects):
        if 'rect_right4' in planted:
            x2 = x2 // 4 * 4
        if x2 > x1 and y2 > y1:
            res[y1:y2, x1:x2] = outs[k][y1:y2, x1:x2]
    return res


def acc_weight(i):
    """a float32 Dirichlet-like weight, one per launch number"""
    w = np.random.RandomState(1000 + i).dirichlet([1.0] * 3).astype(f32)
    return f32(w[i % 3])


# ------------------------------------------------------------------------------------------------------------ scripted draws
class Script:
    """A prescribed list of draws in place of a numpy RandomState: floats are unit doubles (``uniform(low, high)`` returns
    low + (high - low) * u like numpy's legacy generator, ``beta`` returns its value as it is), ints answer ``choice``."""

    def __init__(self, values):
        self.values, self.pos = list(values), 0

    def _next(self, kind):
        assert self.pos < len(self.values), 'more draws than scripted'
        v = self.values[self.pos]
        self.pos += 1
        assert isinstance(v, kind) and not isinstance(v, bool), (self.pos - 1, v, kind)
        return v

    def done(self):
        return self.pos == len(self.values)

    def choice(self, n):
        v = self._next(int)
        assert 0 <= v < n
        return v

    def uniform(self, low=0.0, high=1.0):
        return low + (high - low) * self._next(float)

    def random(self):
        return self._next(float)

    rand = random

    def random_sample(self, n):
        return np.array([self._next(float) for _ in range(n)], np.float64)

    def beta(self, a, b):
        return self._next(float)

    def patch_numpy(self, monkeypatch):
        """route the ``np.random`` functions the oracle calls to this script"""
        for name in ('choice', 'uniform', 'random', 'rand', 'random_sample', 'beta'):
            monkeypatch.setattr(np.random, name, getattr(self, name))


def warp_scripts(aug_list):
    """section B: [(label, draws)] for ``aug`` - the op's index, then its own draws in the order the transform takes them"""
    out = []
    inv = aug_list.index('invert')
    for tx in (U_PLUS, U_MINUS):
        for ty in (U_PLUS, U_MINUS):
            out.append((f'invert tx{tx} ty{ty}', [inv, tx, ty]))
    for kind in GEO_KINDS:
        if kind == 'rotate':
            head = [aug_list.index('bg_only_rotate')]
        else:
            head = [aug_list.index(f'bg_only_{kind[:-2]}_xy'), 0.25 if kind.endswith('_x') else 0.75]
        for sign in (U_PLUS, U_MINUS):
            for u in (U_LOW, U_MID, U_HIGH):
                out.append((f'bg {kind} u{u} sign{sign}', head + [u, sign]))
    return out


def mask_variants(H, W):
    """section B's gt boxes: none, one full-image box, three overlapping boxes with fractional corners"""
    v = [('no_box', np.zeros((0, 4), np.float32))]
    if H >= 4 and W >= 4:           # below that the quarter-resolution mask has no rows: the reference cannot build it
        v.append(('full_box', np.array([[0, 0, W, H]], np.float32)))
        v.append(('three_boxes', np.array([[0.3 * W, 0.2 * H, 0.8 * W + 0.4, 0.7 * H + 0.3],
                                           [0.1 * W + 0.6, 0.4 * H + 0.1, 0.6 * W, 0.9 * H + 0.2],
                                           [0.5 * W + 0.2, 0.1 * H + 0.7, W - 0.5, 0.6 * H]], np.float32)))
    return v


def box_sets(H, W):
    """section C's gt box sets"""
    return [
        ('full', np.array([[0, 0, W, H]], np.float32)),
        ('bottom_right', np.array([[W - 20.5, H - 13.25, W, H]], np.float32)),
        ('thin', np.array([[8.5, 5, 11.5, 25]], np.float32)),                 # quarter-resolution columns 2..2: empty mask
        ('no_width', np.array([[20.25, 5, 20.75, 30]], np.float32)),          # int width 0: no draw
        ('two_levels', np.array([[6, 4, 34, 26], [20, 12, 52, 31]], np.float32)),
        ('fractional', np.array([[5.7, 3.2, 41.9, 28.6], [W - 24.3, 1.5, W - 2.1, 19.8]], np.float32)),
    ]


def box_draws(gts, u_level, u_sign):
    """section C: (level, sign) per box that draws; the second box takes the other extreme and the other sign"""
    d = []
    k = 0
    for g in gts:
        x1, y1, x2, y2 = (int(v) for v in g)
        if x2 - x1 < 1 or y2 - y1 < 1:
            continue
        if k % 2 == 0:
            d += [u_level, u_sign]
        else:
            d += [U_HIGH if u_level == U_LOW else U_LOW, U_MINUS if u_sign == U_PLUS else U_PLUS]
        k += 1
    return d


# ------------------------------------------------------------------------------------------------------------ final mix
@functools.lru_cache(maxsize=None)
def mix_inputs(H, W):
    """section D: (img, acc) - ``acc`` holds exact 0, exact 255 and 255.00003 under pixels of value 255"""
    rs = _rs('mix', H, W)
    img = image('noise', H, W).copy()
    acc = rs.uniform(0, 255, (H, W, 3)).astype(f32)
    img[0:4, 0:6] = 255
    acc[0:4, 0:2] = f32(255.00003)
    acc[0:4, 2:4] = f32(255.0)
    acc[0:4, 4:6] = f32(0.0)
    img[H - 3:, W - 5:] = 0
    acc[H - 3:, W - 5:] = f32(0.0)
    img[H // 2, :] = 255
    acc[H // 2, :] = f32(255.00003)
    for a in (img, acc):
        a.setflags(write=False)
    return img, acc


def mix_targets(H, W):
    """section D's target sets: [(name, [('rect', [x1, y1, x2, y2]) | ('fg', box)] ...)]"""
    fg_a = [0.15 * W, 0.1 * H, 0.7 * W + 0.5, 0.75 * H + 0.25]
    fg_b = [0.4 * W + 0.5, 0.35 * H, 0.95 * W, 0.9 * H + 0.5]
    small = [('rect', [x, y, x + 2, y + 2]) for y in range(0, 14, 2) for x in range(0, 20, 2)]
    assert len(small) == 70
    return [
        ('none', []),
        ('whole', [('rect', [0, 0, W, H])]),
        ('three_identical', [('rect', [2, 1, W - 3, H - 2])] * 3),
        ('fg_fg_rect', [('fg', fg_a), ('fg', fg_b), ('rect', [W // 4, H // 3, W - 2, H // 3 + 5])]),
        ('seventy_small', small),
    ]


def mix_units(n, shift):
    """(unit draw, score) per target: the m_oa units in turn; 0.99999994 needs a score above the threshold (hi = 1)"""
    out = []
    for t in range(n):
        u = M_OA_UNITS[(t + shift) % 3]
        if u == M_OA_UNITS[2]:
            out.append((u, 11.0))
        else:
            out.append((u * 2, -1) if (t + shift) % 2 else (u, float('inf')))       # hi = 0.5 and hi = 1 give the same m_oa
    return out


def final_mix(img, acc, masks, m_oas, m_beta, planted=()):
    """final_mix_kernel's arithmetic: masks [H, W] float32 each, m_oas float32 each; returns the uint8 view and the number of
    values the final clip changed"""
    im, ag = img.astype(f32), acc.astype(f32)
    H, W = img.shape[:2]
    orig, aug = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    mask_sum, mask_max = np.zeros((H, W, 1), f32), None
    for j, (mask, m_oa) in enumerate(zip(masks, m_oas)):
        mask, m_oa = mask.astype(f32)[..., None], f32(m_oa)
        mask_sum = mask_sum + mask
        mask_max = mask if j == 0 else np.maximum(mask_max, mask)
        wgt = mask - (mask_sum - mask_max) * f32(0.5)
        orig = orig + ((f32(1.0) - m_oa) * im) * wgt
        aug = aug + (m_oa * ag) * wgt
        mask_sum = mask_max
    rest = f32(1.0) - mask_sum
    m = float(m_beta)
    if 'rest_moa' in planted and len(m_oas):
        m = float(m_oas[-1])
    o = orig + aug
    o = (o.astype(np.float64) + ((1.0 - m) * img.astype(np.float64)) * rest.astype(np.float64)).astype(f32)
    o = o + (f32(m) * ag) * rest
    clipped = int(((o < 0) | (o > 255)).sum())
    return np.clip(o, 0, 255).astype(np.uint8), clipped


def normalized(u8, to_rgb):
    """mmcv.imnormalize in float32: (channel-swapped u8 - mean) * (1 / std)"""
    mean = np.array(MEAN, f32)
    stdinv = (1.0 / np.array(STD, np.float64)).astype(f32)
    src = u8[..., ::-1] if to_rgb else u8
    return (src.astype(f32) - mean) * stdinv
