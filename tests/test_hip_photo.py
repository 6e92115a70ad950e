"""GPU: oadg_photo_normalize_batch (csrc/photo.hip) through its wrapper oadg_photo.photo_normalize_batch - the suite that
answers for that C-ABI call site.  The judge is the numpy restatement of tests/test_photometric.py, which reproduces every
output of the genuine reference classes in tests/golden/photometric_reference.npz bit for bit.  Gate: the project's fp32
parity bound (README.md), |got - want| <= 1e-4 * max(1, |want|) on the normalised values; every operation of the kernel is a
correctly rounded fp32 operation in the restatement's order, so bit identity is expected and the number of elements that are
not bit-identical is printed.  Outputs are prefilled with NaN: the pad region must come back exactly 0."""
import numpy as np
import pytest
import torch

import test_photometric as TP
from test_photometric import FORCED, SEEDED, bits, case_image, case_params, cutout_cases, normalize, restate

gpu = pytest.mark.gpu
g = TP.g                                         # the fixture file (module-scoped pytest fixture)


def pads(H, W):
    """(H, W), (H + 3, W + 5) and the size_divisor = 32 extents"""
    return [(H, W), (H + 3, W + 5), (-(-H // 32) * 32, -(-W // 32) * 32)]


def launch(dev, images, samples, to_rgb, Hp, Wp, dtype=torch.float32):
    """one launch on NaN-prefilled output -> the [N, Hp, Wp, 3] tensor"""
    import oadg_photo
    mean, stdinv = TP.norm_args()
    out = torch.full((len(images), Hp, Wp, 3), float('nan'), dtype=dtype, device=dev)
    d_imgs = [torch.from_numpy(np.ascontiguousarray(im)).to(dev) for im in images]
    got = oadg_photo.photo_normalize_batch(d_imgs, samples, mean, stdinv, to_rgb, out)
    assert got is out
    return out


def expect(images, samples, to_rgb, Hp, Wp):
    mean, stdinv = TP.norm_args()
    return np.stack([restate(im, s['photo'], s['rects'], s['fill'], s['cutout_last'], mean, stdinv, to_rgb, Hp, Wp)
                     for im, s in zip(images, samples)])


def judge(got, want, what):
    """the gate; -> elements that are not bit-identical"""
    got = got.float().cpu().numpy()
    assert not np.isnan(got).any(), f'{what}: NaN left in the output'
    err = np.abs(got - want)
    bound = 1e-4 * np.maximum(1.0, np.abs(want))
    assert (err <= bound).all(), (what, float((err / bound).max()), float(err.max()))
    return int((bits(got) != bits(want)).sum())


def fixture_groups(g):
    """the fixture's cases as batches of equally sized images: [(name, images, sample records, reference floats or None)]"""
    import oadg_photo
    from oadg_amd.pipelines.photometric import CutOut
    groups = []
    for name, tags in (('forced', FORCED), ('seeded A', SEEDED[0::3]), ('seeded ONE', SEEDED[1::3]), ('seeded B', SEEDED[2::3])):
        groups.append((name, [case_image(g, t) for t in tags], [oadg_photo.sample(case_params(g, t)) for t in tags],
                       [g[t + '_out'] for t in tags]))
    for tag, name, seed, kw in cutout_cases(g):
        rects = g[f'cutout_{tag}_rects']
        if name == 'F':     # the reference's CutOut on the float output of PhotoMetricDistortion seed 0: CutOut LAST
            s = oadg_photo.sample(case_params(g, 'seed0'), rects, CutOut(**kw).fill(on_uint8=False), cutout_last=True)
            groups.append((f'cutout {tag}', [g['A']], [s], [g[f'cutout_{tag}_out']]))
        else:
            s = oadg_photo.sample(None, rects, CutOut(**kw).fill(on_uint8=True))
            groups.append((f'cutout {tag}', [g[name]], [s], [g[f'cutout_{tag}_out'].astype(np.float32)]))
    return groups


@gpu
@pytest.mark.parametrize('to_rgb', [0, 1])
def test_kernel_reproduces_every_fixture_case(dev, g, to_rgb):
    """every PhotoMetricDistortion and CutOut case of the fixture with forced parameters, fp32: against the restatement
    (the gate) and, through Normalize by hand, against the reference's own output floats"""
    mean, stdinv = TP.norm_args()
    off_by_bits, n = 0, 0
    for name, images, samples, ref in fixture_groups(g):
        H, W = images[0].shape[:2]
        for Hp, Wp in pads(H, W):
            got = launch(dev, images, samples, to_rgb, Hp, Wp)
            want = expect(images, samples, to_rgb, Hp, Wp)
            theirs = np.stack([normalize(r, mean, stdinv, to_rgb, Hp, Wp) for r in ref])
            assert np.array_equal(bits(want), bits(theirs)), name        # the restatement IS the reference's output
            off_by_bits += judge(got, want, f'{name} pad {Hp} x {Wp} to_rgb {to_rgb}')
            n += want.size
            pad = got.cpu().numpy().copy()
            pad[:, :H, :W] = 0
            assert not pad.any(), f'{name}: the pad region is not exactly 0'
    print(f'photo kernel vs restatement, to_rgb {to_rgb}: {off_by_bits} of {n} elements not bit-identical')


@gpu
def test_bf16_output_is_the_fp32_output_rounded(dev, g):
    """same launches in bf16: bit for bit torch's .to(bfloat16) of the fp32 result (round to nearest even both: f32_to_bf16
    is the hardware conversion); wide stores (Wp % 4 == 0) and element stores alike"""
    for name, images, samples, _ in fixture_groups(g):
        H, W = images[0].shape[:2]
        for Hp, Wp in pads(H, W):
            f = launch(dev, images, samples, 1, Hp, Wp)
            h = launch(dev, images, samples, 1, Hp, Wp, dtype=torch.bfloat16)
            assert not torch.isnan(h.float()).any()
            assert torch.equal(h.view(torch.int16), f.to(torch.bfloat16).view(torch.int16)), (name, Hp, Wp)


def _plain_normalize(dev, img_u8, to_rgb, Hp, Wp, dtype):
    from oadg_amd import _lib
    mean, stdinv = TP.norm_args()
    import ctypes
    out = torch.full((Hp, Wp, 3), float('nan'), dtype=dtype, device=dev)
    d = torch.from_numpy(np.ascontiguousarray(img_u8)).to(dev)
    H, W = img_u8.shape[:2]
    _lib.check(_lib.lib().oadg_oamix_normalize(_lib.ptr(d), H, W, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*stdinv),
                                               to_rgb, _lib.ptr(out), 1 if dtype == torch.bfloat16 else 0, Hp, Wp,
                                               _lib.stream_ptr()), 'oadg_oamix_normalize')
    return out


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_cutout_only_is_the_plain_normalize_of_the_filled_image(dev, g, dtype):
    """no photometric step: the bits of oadg_oamix_normalize on the uint8 image whose holes torch indexing filled -
    0 holes, 70 (overlapping) holes, holes that overlap by construction"""
    import oadg_photo
    overlapping = np.array([[3, 2, 20, 12], [10, 5, 30, 9], [10, 5, 30, 9], [0, 0, 53, 1], [52, 36, 53, 37]], np.int32)
    for img, rects, fill in ((g['A'], np.zeros((0, 4), np.int32), (7, 8, 9)), (g['B'], g['cutout_seventy_rects'], (9, 9, 9)),
                             (g['A'], overlapping, (0, 255, 128)), (g['ONE'], g['cutout_pixel_rects'], (5, 6, 7))):
        H, W = img.shape[:2]
        filled = torch.from_numpy(img.copy())
        for x1, y1, x2, y2 in rects.tolist():
            filled[y1:y2, x1:x2] = torch.tensor(fill, dtype=torch.uint8)
        for Hp, Wp in pads(H, W):
            for to_rgb in (0, 1):
                got = launch(dev, [img], [oadg_photo.sample(None, rects, fill)], to_rgb, Hp, Wp, dtype)[0]
                want = _plain_normalize(dev, filled.numpy(), to_rgb, Hp, Wp, dtype)
                assert not torch.isnan(got.float()).any()
                assert torch.equal(got.view(torch.int32 if dtype == torch.float32 else torch.int16),
                                   want.view(torch.int32 if dtype == torch.float32 else torch.int16)), (H, W, Hp, Wp, to_rgb)


@gpu
def test_cutout_before_and_after_the_photometric_step(dev, g):
    """the two orders differ on the hole pixels and nowhere else; each matches its restatement"""
    import oadg_photo
    img, p = g['A'], case_params(g, 'forced_m1_31')                     # every sub-step on
    rects, fill = np.array([[5, 3, 25, 20], [20, 15, 53, 37], [0, 30, 4, 30]], np.int32), (12.5, 0.25, 250.75)
    hole = np.zeros(img.shape[:2], bool)
    for x1, y1, x2, y2 in rects:
        hole[y1:y2, x1:x2] = True
    out = {}
    for last in (False, True):
        s = [oadg_photo.sample(p, rects, fill, cutout_last=last)]
        got = launch(dev, [img], s, 1, 64, 64)
        off = judge(got, expect([img], s, 1, 64, 64), f'cutout_last {last}')
        print(f'cutout_last {last}: {off} elements not bit-identical')
        out[last] = got[0, :37, :53].cpu().numpy()
    differs = (out[False] != out[True]).any(-1)
    assert hole.any() and differs[hole].all() and not differs[~hole].any()


@gpu
def test_a_batch_of_three_shapes_equals_three_single_launches(dev, g):
    """37 x 53, 1 x 1 and 32 x 64 in ONE launch into one [3, Hp, Wp, 3] tensor, each image with its own parameters, holes
    and order: bit for bit the three single-image launches"""
    import oadg_photo
    images = [g['A'], g['ONE'], g['B']]
    samples = [oadg_photo.sample(case_params(g, 'seed0'), g['cutout_ratio_rects'], (10, 200, 30)),
               oadg_photo.sample(case_params(g, 'seed4'), g['cutout_pixel_rects'], (1.5, 2.5, 3.5), cutout_last=True),
               oadg_photo.sample(None, g['cutout_seventy_rects'], (9, 9, 9))]
    for dtype, as_int in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
        for Hp, Wp in ((37, 64), (40, 69), (64, 64)):
            both = launch(dev, images, samples, 1, Hp, Wp, dtype)
            assert not torch.isnan(both.float()).any()
            for i in range(3):
                single = launch(dev, images[i:i + 1], samples[i:i + 1], 1, Hp, Wp, dtype)
                assert torch.equal(both[i].view(as_int), single[0].view(as_int)), (dtype, Hp, Wp, i)
            if dtype == torch.float32:
                judge(both, expect(images, samples, 1, Hp, Wp), f'batch {Hp} x {Wp}')


PIPE = [dict(type='Resize', img_scale=[(128, 50), (128, 64)], keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.5),
        dict(type='PhotoMetricDistortion'),
        dict(type='CutOut', n_holes=(1, 5), cutout_ratio=[(0.1, 0.2), (0.25, 0.1)], fill_in=(12.5, 0.25, 250.75))] + TP.TAIL


@gpu
def test_device_pipeline_with_both_steps(dev):
    """[Resize, RandomFlip, PhotoMetricDistortion, CutOut, Normalize, Pad, ...] on two seeded 64 x 128 images with boxes: the
    image tensor is the restatement applied to the repository's own Resize / Flip outputs under the same seed, with the draws
    made by hand in the reference's per-sample order; boxes, generator state and meta keys as without the two steps"""
    from inputs import lowpass_image, synthetic_boxes
    from oadg_amd.pipelines import Compose, DevicePipeline
    from oadg_amd.pipelines.oa_mix import rng
    rs = np.random.RandomState(11)
    imgs = torch.from_numpy(np.stack([lowpass_image(rs, 64, 128) for _ in range(2)])).to(dev)
    boxes = [synthetic_boxes(rs, 4, 64, 128, 6, 32) for _ in range(2)]
    labels = [np.arange(4, dtype=np.int64) for _ in range(2)]
    mean, stdinv = TP.norm_args()
    for seed in (3, 4):
        np.random.seed(seed)
        out = DevicePipeline(PIPE)(imgs, boxes, labels)
        after = rng.uniform()
        # by hand
        np.random.seed(seed)
        resize, flip, photo, cutout = Compose(PIPE[:4]).transforms
        want, want_boxes, shapes = [], [], []
        for i in range(2):
            im, bx, _ = resize(imgs[i], boxes[i])
            im, bx, _ = flip(im, bx)
            p = photo.draw()
            r = cutout.draw(int(im.shape[0]), int(im.shape[1]))
            want.append((im.cpu().numpy(), p, r))
            want_boxes.append(bx)
            shapes.append(tuple(im.shape[:2]))
        assert rng.uniform() == after
        Hp, Wp = out['img'].shape[2:]
        assert (Hp, Wp) == (max(-(-h // 32) * 32 for h, _ in shapes), max(-(-w // 32) * 32 for _, w in shapes))
        got = out['img'].permute(0, 2, 3, 1)
        assert got.is_contiguous()
        exp = np.stack([restate(im, p, r, cutout.fill(on_uint8=False), True, mean, stdinv, True, Hp, Wp) for im, p, r in want])
        print('pipeline seed %d: %d elements not bit-identical' % (seed, judge(got, exp, f'pipeline seed {seed}')))
        for i in range(2):
            assert np.array_equal(out['gt_bboxes'][i].cpu().numpy(), want_boxes[i])
            assert out['img_metas'][i]['img_shape'] == shapes[i] + (3,)
        np.random.seed(seed)
        plain = DevicePipeline(PIPE[:2] + TP.TAIL)(imgs, boxes, labels)
        assert [sorted(m) for m in out['img_metas']] == [sorted(m) for m in plain['img_metas']]
        assert sorted(out) == sorted(plain)


@gpu
def test_wrapper_refuses_what_it_cannot_run(dev, g):
    import oadg_photo
    mean, stdinv = TP.norm_args()
    img = torch.from_numpy(g['B'].copy())
    d_img = img.to(dev)
    ok = torch.empty((1, 32, 64, 3), device=dev)
    s = [oadg_photo.sample()]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        oadg_photo.photo_normalize_batch([img], s, mean, stdinv, 1, ok)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        oadg_photo.photo_normalize_batch([d_img], s, mean, stdinv, 1, ok.cpu())
    with pytest.raises(ValueError, match='float32 or bfloat16'):
        oadg_photo.photo_normalize_batch([d_img], s, mean, stdinv, 1, ok.half())
    with pytest.raises(ValueError, match='uint8'):
        oadg_photo.photo_normalize_batch([d_img.float()], s, mean, stdinv, 1, ok)
    with pytest.raises(ValueError, match='contiguous'):
        oadg_photo.photo_normalize_batch([d_img], s, mean, stdinv, 1, torch.empty((1, 3, 32, 64), device=dev).permute(0, 2, 3, 1))
    with pytest.raises(ValueError, match='contiguous'):
        oadg_photo.photo_normalize_batch([d_img[:, ::2]], s, mean, stdinv, 1, ok)
    with pytest.raises(ValueError, match='does not fit'):
        oadg_photo.photo_normalize_batch([d_img], s, mean, stdinv, 1, torch.empty((1, 32, 63, 3), device=dev))
    with pytest.raises(ValueError, match='int32'):
        oadg_photo.photo_normalize_batch([d_img], [oadg_photo.sample(rects=np.zeros((1, 4), np.int64))], mean, stdinv, 1, ok)
    with pytest.raises(ValueError, match='permutation'):
        p = dict(case_params(g, 'seed0'), perm=(0, 0, 2))
        oadg_photo.photo_normalize_batch([d_img], [oadg_photo.sample(p)], mean, stdinv, 1, ok)
    with pytest.raises(ValueError, match='2 were given'):
        oadg_photo.photo_normalize_batch([d_img, d_img], s * 2, mean, stdinv, 1, ok)
