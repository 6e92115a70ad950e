"""CPU: the device route of Corrupt.batch for jpeg_compression and pixelate (csrc/recompress.hip, oadg_recompress.py) as
far as it goes without a GPU.  The kernels' source runs on numpy buffers through the host twins (oadg_jpeg_recompress_host,
oadg_pil_pixelate_host) and must equal ``corrupt()`` - Pillow on this machine - byte for byte; the tables the wrapper
uploads (libjpeg's quantisation tables, Pillow's BOX coefficients and NEAREST scan) are checked against Pillow on their
own, the saturation rule on hand-built blocks, and the routing as far as a CPU batch shows it.  The bytes on the GPU are
tests/test_hip_recompress.py's."""
import os
import re
from io import BytesIO

import numpy as np
import pytest

from inputs import lowpass_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEVERITIES = (1, 2, 3, 4, 5)
JPEG_SIZES = [(1, 1), (2, 2), (2, 4), (4, 2), (1, 7), (7, 1), (3, 5), (5, 3),        # chroma at most 2 wide: replication
              (8, 8), (16, 16), (9, 13), (17, 33), (31, 17),
              (40, 56), (42, 58), (24, 40), (34, 50), (18, 6),      # even, no multiple of 16: the bottom edge is padded late
              (61, 97), (130, 254), (64, 48)]
PIXELATE_SIZES = [(4, 4), (5, 7), (9, 13), (33, 47), (40, 56), (61, 97), (130, 254), (256, 512)]


def contents(h, w):
    """uniform noise, a lowpass image, 0 / 255 noise, a constant 128 image, a one-pixel checkerboard"""
    rs = np.random.RandomState(1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, 2)
    return np.stack([rs.randint(0, 256, (h, w, 3)).astype(np.uint8), lowpass_image(rs, h, w, 4),
                     (rs.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8), np.full((h, w, 3), 128, np.uint8), checker])


def _first_difference(out, ref):
    bad = np.argwhere(out != ref)
    return len(bad), bad[:5].tolist(), [(int(out[tuple(b)]), int(ref[tuple(b)])) for b in bad[:5]]


@pytest.mark.parametrize('h,w', JPEG_SIZES)
def test_jpeg_host_twin_equals_pillow(h, w):
    import oadg_recompress as R
    from oadg_amd.pipelines.corrupt import corrupt
    imgs = contents(h, w)
    for s in SEVERITIES:
        out, flags = R.jpeg_recompress_host(imgs, R.JPEG_QUALITY[s - 1])
        ref = np.stack([corrupt(im, 'jpeg_compression', s) for im in imgs])
        assert np.array_equal(out, ref), (h, w, s) + _first_difference(out, ref)
        assert not flags.any(), (h, w, s, flags.tolist())


@pytest.mark.parametrize('h,w', PIXELATE_SIZES)
def test_pixelate_host_twin_equals_pillow(h, w):
    import oadg_recompress as R
    from oadg_amd.pipelines.corrupt import corrupt
    imgs = contents(h, w)[:2]
    for s in SEVERITIES:
        oh, ow = R.pixelate_size(h, w, s)
        out = R.pixelate_host(imgs, oh, ow)
        ref = np.stack([corrupt(im, 'pixelate', s) for im in imgs])
        assert np.array_equal(out, ref), (h, w, s) + _first_difference(out, ref)


def test_pixelate_of_a_3x3_image_is_declined_and_pillow_raises():
    import torch
    import oadg_recompress as R
    from oadg_amd.pipelines.corrupt import Corrupt, corrupt
    img = np.full((3, 3, 3), 9, np.uint8)
    assert R.pixelate_size(3, 3, 5) == (0, 0)
    assert R.corrupt_batch(torch.from_numpy(img[None]), 'pixelate', 5) is None
    with pytest.raises(ValueError):
        corrupt(img, 'pixelate', 5)
    with pytest.raises(ValueError):
        Corrupt('pixelate', 5).batch(torch.from_numpy(img[None]))
    with pytest.raises(ValueError):
        R.box_tables(3, 0)


# ------------------------------------------------------------------------------------------------------------ the tables
def _apply_box(line, bounds, coeffs):
    """[n_in, 3] uint8 -> [n_out, 3]: Pillow's 8-bit resampling sum with the uploaded tables"""
    out = np.empty((len(bounds), 3), np.uint8)
    for i, (lo, cnt) in enumerate(bounds):
        acc = (1 << 21) + (line[lo:lo + cnt].astype(np.int64) * coeffs[i, :cnt, None].astype(np.int64)).sum(0)
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


@pytest.mark.parametrize('n_in,n_out', [(2048, 1228), (1024, 256), (97, 58), (2048, 512), (1024, 614), (61, 15), (7, 1),
                                        (254, 76), (5, 3), (13, 13)])
def test_box_and_nearest_tables_are_pillows(n_in, n_out):
    from PIL import Image
    import oadg_recompress as R
    rs = np.random.RandomState(n_in + n_out)
    line = rs.randint(0, 256, (n_in, 3)).astype(np.uint8)
    bounds, coeffs = R.box_tables(n_in, n_out)
    assert bounds.dtype == np.int32 and coeffs.dtype == np.int32 and coeffs.shape[0] == n_out
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= coeffs.shape[1]).all()
    mine = _apply_box(line, bounds, coeffs)
    across = np.asarray(Image.fromarray(line[None]).resize((n_out, 1), Image.BOX))[0]
    down = np.asarray(Image.fromarray(line[:, None]).resize((1, n_out), Image.BOX))[:, 0]
    assert np.array_equal(mine, across) and np.array_equal(mine, down)
    # NEAREST back up: n_out -> n_in
    idx = R.nearest_table(n_out, n_in)
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < n_out
    up = np.asarray(Image.fromarray(mine[None]).resize((n_in, 1), Image.NEAREST))[0]
    assert np.array_equal(mine[idx], up)
    up = np.asarray(Image.fromarray(mine[:, None]).resize((1, n_in), Image.NEAREST))[:, 0]
    assert np.array_equal(mine[idx], up)


def test_nearest_scan_accumulates():
    """the scan adds its step output by output; the closed form int((i + 0.5) * a) is another table at some sizes - and
    Pillow's bytes are the accumulating one's (test above)"""
    import oadg_recompress as R
    differ = 0
    for n_in, n_out in [(614, 1024), (1228, 2048), (58, 97), (76, 254), (307, 1024)]:
        a = n_in / n_out
        closed = np.array([int((i + 0.5) * a) for i in range(n_out)], np.int32)
        differ += int((closed != R.nearest_table(n_in, n_out)).sum())
    print('outputs where the closed form differs from the accumulating scan:', differ)
    xo, a, want = 0.5 * (58 / 97), 58 / 97, []
    for _ in range(97):
        want.append(int(xo))
        xo += a
    assert R.nearest_table(58, 97).tolist() == want


@pytest.mark.parametrize('quality', [25, 18, 15, 10, 7, 50, 75, 95, 1, 100])
def test_quantisation_tables_are_the_ones_pillow_writes(quality):
    from PIL import Image
    import oadg_recompress as R
    buf = BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, 'JPEG', quality=quality)
    im = Image.open(buf)
    mine = R.quant_tables(quality)
    assert mine.dtype == np.uint16 and mine.shape == (2, 64) and mine.min() >= 1
    # Image.quantization holds the tables in natural (row-major) order; the file holds them in zig-zag order
    theirs = [np.asarray(im.quantization[k]) for k in (0, 1)]
    for k in (0, 1):
        assert np.array_equal(mine[k], theirs[k]), (quality, k)
    if 7 <= quality <= 95:
        assert mine[0, 5] > mine[0, 40]                      # natural order: (v 0, u 5) is 40, (v 5, u 0) is 24 in table K.1


def test_severities_use_the_host_paths_parameters():
    import inspect
    import oadg_recompress as R
    from oadg_amd.pipelines import corrupt as C
    assert str(list(R.JPEG_QUALITY)) in inspect.getsource(C.jpeg_compression)
    assert str(list(R.PIXELATE_SCALE)) in inspect.getsource(C.pixelate)
    assert R.NAMES == C.DEVICE_CODEC_CORRUPTIONS


# ------------------------------------------------------------------------------------------------------ the saturation rule
def _dc(value):
    block = np.zeros(64, np.int32)
    block[0] = value
    return block


def test_saturation_bounds_just_inside_and_just_outside():
    """A DC coefficient c alone gives column-pass values 4 c and samples (4 c + 16) >> 5 (descaling by 11, then by 18).
    Column pass: -4095 -> -16380 (inside), -4096 -> -16384 (outside) with samples of -512, still inside theirs.
    Samples: 4091 -> 511 (inside), 4092 -> 512 (outside) with column-pass values of 16368, inside theirs.
    Coefficients: 16383 is inside its own bound, 16384 outside; the later bounds are broken either way (a column pass has
    gain 4 at least, so the first bound cannot be the only one broken)."""
    import oadg_recompress as R
    f = R.idct_bounds_host
    assert f(np.zeros(64, np.int32)) == 0
    assert f(_dc(-4095)) == 0 and f(_dc(-4096)) == R.BOUND_COLUMN
    assert f(_dc(4091)) == 0 and f(_dc(4092)) == R.BOUND_SAMPLE
    for sign in (1, -1):
        assert f(_dc(sign * 16383)) & R.BOUND_COEF == 0 and f(_dc(sign * 16383)) & R.BOUND_COLUMN
        assert f(_dc(sign * 16384)) == R.BOUND_COEF | R.BOUND_COLUMN | R.BOUND_SAMPLE
    # the same along the other axes of the block: the highest horizontal, the highest vertical frequency
    for k in (56, 7, 63):
        block = np.zeros(64, np.int32)
        block[k] = 16384
        assert f(block) & R.BOUND_COEF
        block[k] = 16383
        assert f(block) & R.BOUND_COEF == 0
    # a sample bound broken by many small coefficients, none near its own bound
    block = np.zeros(64, np.int32)
    block[[0, 8, 16, 24]] = 1400
    assert f(block) == R.BOUND_SAMPLE
    block[[0, 8, 16, 24]] = 700
    assert f(block) == 0
    with pytest.raises(ValueError):
        f(np.zeros(63, np.int32))


def test_worst_values_on_the_test_contents_stay_far_inside():
    """no content of these tests flags an image at any severity (the condition of the GPU tests: zero fall-backs)"""
    import oadg_recompress as R
    for h, w in [(61, 97), (40, 56), (64, 48)]:
        for q in R.JPEG_QUALITY:
            assert not R.jpeg_recompress_host(contents(h, w), q)[1].any()


# ------------------------------------------------------------------------------------------------------------- the routing
def test_c_abi_carries_the_entry_points_with_the_stream_last():
    from oadg_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'oadg_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(oadg_(?:jpeg_recompress|pil)_[a-z0-9_]+)\s*\(', src))
    assert declared == {'oadg_jpeg_recompress_u8', 'oadg_jpeg_recompress_workspace_bytes', 'oadg_jpeg_recompress_host',
                        'oadg_jpeg_recompress_bounds_host', 'oadg_pil_box_resize_u8', 'oadg_pil_nearest_u8',
                        'oadg_pil_pixelate_host'}
    assert declared <= set(_lib.SIGNATURES)
    for name in ('oadg_jpeg_recompress_u8', 'oadg_pil_box_resize_u8', 'oadg_pil_nearest_u8'):
        assert _lib.SIGNATURES[name][1][-1] is _lib.vp, name
    L = _lib.lib()
    assert L.oadg_jpeg_recompress_workspace_bytes(2, 40, 56) == 2 * 3 * 4 * 6 * 64
    assert L.oadg_jpeg_recompress_workspace_bytes(1, 1024, 2048) == 1024 * 2048 * 3 // 2
    assert L.oadg_jpeg_recompress_workspace_bytes(0, 8, 8) == 0


def test_package_never_spells_the_c_symbols():
    """the ctypes calls live in oadg_recompress.py, next to the import shim (tests/test_target_audit.py's closure)"""
    for dp, _, files in os.walk(os.path.join(ROOT, 'oa-dg_amd')):
        for f in files:
            if f.endswith('.py'):
                assert not re.search(r'\.oadg_(jpeg_recompress|pil_)', open(os.path.join(dp, f)).read()), os.path.join(dp, f)
    src = open(os.path.join(ROOT, 'oadg_recompress.py')).read()
    assert 'tests/test_hip_recompress.py' in src
    for name in ('oadg_jpeg_recompress_u8', 'oadg_jpeg_recompress_workspace_bytes', 'oadg_jpeg_recompress_host',
                 'oadg_pil_box_resize_u8', 'oadg_pil_nearest_u8', 'oadg_pil_pixelate_host'):
        assert '.' + name + '(' in src, name


def test_codec_names_are_host_names_with_a_device_route():
    from oadg_amd.pipelines import corrupt as C
    assert C.DEVICE_CODEC_CORRUPTIONS == ('pixelate', 'jpeg_compression')
    assert set(C.DEVICE_CODEC_CORRUPTIONS) <= set(C.HOST_CORRUPTIONS)
    assert not set(C.DEVICE_CODEC_CORRUPTIONS) & set(C.DEVICE_CORRUPTIONS)
    from oadg_amd.pipelines import corrupt_device as D
    assert not set(C.DEVICE_CODEC_CORRUPTIONS) & set(D._DEVICE_FUNCS)


@pytest.mark.parametrize('name', ['pixelate', 'jpeg_compression'])
def test_a_cpu_batch_takes_the_host_path_and_is_counted(name, monkeypatch):
    import torch
    import oadg_recompress as R
    from oadg_amd.pipelines.corrupt import Corrupt, corrupt

    def never(*a, **k):
        raise AssertionError('a CPU batch reached the device route')
    monkeypatch.setattr(R, 'corrupt_batch', never)
    rs = np.random.RandomState(3)
    imgs = rs.randint(0, 256, (2, 11, 17, 3)).astype(np.uint8)
    before = dict(Corrupt.runs)
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    out = Corrupt(name, 2).batch(torch.from_numpy(imgs))
    assert not out.is_cuda and out.dtype == torch.uint8
    assert Corrupt.runs['host'] == before['host'] + 2 and Corrupt.runs['device'] == before['device']
    assert np.array_equal(out.numpy(), np.stack([corrupt(im, name, 2) for im in imgs]))
    assert np.array_equal(np.random.get_state()[1], state)          # neither name draws
