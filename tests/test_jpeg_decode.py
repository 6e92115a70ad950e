"""csrc/jpeg_decode.hip against PIL (libjpeg-turbo under its defaults = OpenCV's cv2.imdecode, the reference's
LoadImageFromFile): the host twin on the CPU, the device pixel stage batched as CocoDataset.batch batches it on the GPU.
JPEGs are written at test time by PIL from seeded arrays (lowpass_image + uniform noise)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from inputs import lowpass_image

OK, EARG, ESIZE, EIO, EUNSUPPORTED, EFORMAT = 0, -1, -2, -3, -4, -5
SIZES = [(1, 1), (7, 9), (17, 33), (31, 47), (255, 257), (720, 1280)]
QUALITIES = [10, 50, 75, 95, 100]
SUBSAMPLING = [0, 1, 2, 'L']          # 4:4:4, 4:2:2, 4:2:0, grey
QT16 = [[min(65535, 256 + 37 * i) for i in range(64)], [300 + 5 * i for i in range(64)]]


def _lib():
    from oadg_amd import _lib as lib
    return lib.lib()


def noisy_image(seed, h, w):
    rs = np.random.RandomState(seed)
    a = lowpass_image(rs, h, w, 4).astype(np.int32) + rs.randint(-40, 41, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def write_jpeg(path, seed, h, w, sub, **kw):
    a = noisy_image(seed, h, w)
    from PIL import Image
    if sub == 'L':
        im = Image.fromarray(a[:, :, 1])
        if 'qtables' in kw:
            kw = dict(kw, qtables=kw['qtables'][:1])
    else:
        im = Image.fromarray(a)
        kw = dict(kw, subsampling=sub)
    im.save(path, **kw)
    return str(path)


def pil_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def variants():
    """(name, h, w, subsampling, save kwargs): the whole matrix"""
    out = []
    for (h, w), q, sub in itertools.product(SIZES, QUALITIES, SUBSAMPLING):
        out.append((f'q{q}', h, w, sub, dict(quality=q)))
    for (h, w), sub in itertools.product(SIZES, SUBSAMPLING):
        out += [('opt', h, w, sub, dict(quality=80, optimize=True)),
                ('rstb', h, w, sub, dict(quality=90, restart_marker_blocks=3)),
                ('rstr', h, w, sub, dict(quality=60, restart_marker_rows=1)),
                ('qt16', h, w, sub, dict(qtables=QT16))]
    return out


def write_matrix(tmp_path, sizes=None):
    files = []
    for k, (name, h, w, sub, kw) in enumerate(variants()):
        if sizes is not None and (h, w) not in sizes:
            continue
        files.append((write_jpeg(tmp_path / f'{k}_{name}_{sub}_{h}x{w}.jpg', k, h, w, sub, **kw), h, w))
    return files


def test_matrix_covers_the_markers_it_claims(tmp_path):
    """the generated files really hold what the matrix names: restart markers, 16-bit DQT + SOF1, optimized tables"""
    p = write_jpeg(tmp_path / 'r.jpg', 0, 31, 47, 2, quality=90, restart_marker_blocks=3)
    assert b'\xff\xdd' in open(p, 'rb').read() and b'\xff\xd0' in open(p, 'rb').read()
    p = write_jpeg(tmp_path / 'q.jpg', 0, 31, 47, 0, qtables=QT16)
    raw = open(p, 'rb').read()
    assert b'\xff\xc1' in raw and raw[raw.index(b'\xff\xdb') + 4] >> 4 == 1


def test_host_twin_is_byte_equal_to_pil(tmp_path):
    L = _lib()
    bad = []
    for path, h, w in write_matrix(tmp_path):
        out = np.zeros((h, w, 3), np.uint8)
        rc = L.oadg_jpeg_decode_bgr(path.encode(), out.ctypes.data, h, w)
        if rc != OK or not np.array_equal(out, pil_bgr(path)):
            bad.append((os.path.basename(path), rc))
    assert not bad, bad


def test_size_agrees_with_pil(tmp_path):
    from PIL import Image
    L = _lib()
    a = noisy_image(3, 40, 56)
    Image.fromarray(a).save(tmp_path / 'p.jpg', progressive=True)
    Image.fromarray(a).convert('CMYK').save(tmp_path / 'c.jpg')
    paths = [write_jpeg(tmp_path / f'{h}x{w}.jpg', 1, h, w, 2) for h, w in SIZES] + \
        [str(tmp_path / 'p.jpg'), str(tmp_path / 'c.jpg')]
    for p in paths:
        hh, ww = ctypes.c_int(), ctypes.c_int()
        assert L.oadg_jpeg_size(p.encode(), ctypes.byref(hh), ctypes.byref(ww)) == OK
        with Image.open(p) as im:
            assert (ww.value, hh.value) == im.size, p
    assert L.oadg_jpeg_size(str(tmp_path / 'none.jpg').encode(), ctypes.byref(hh), ctypes.byref(ww)) == EIO


def _patched_411(tmp_path):
    """a 4:4:4 file whose SOF0 luma sampling byte says 4x1: a 4:1:1 header"""
    p = write_jpeg(tmp_path / 'base.jpg', 5, 32, 64, 0, quality=90)
    raw = bytearray(open(p, 'rb').read())
    sof = raw.index(b'\xff\xc0')
    assert raw[sof + 9] == 3 and raw[sof + 10] == 1 and raw[sof + 11] == 0x11    # 3 components; Y: id 1, 1x1
    raw[sof + 11] = 0x41
    q = tmp_path / 'p411.jpg'
    q.write_bytes(bytes(raw))
    return str(q)


def test_declines_and_errors(tmp_path):
    from PIL import Image
    L = _lib()
    a = noisy_image(4, 40, 48)
    Image.fromarray(a).save(tmp_path / 'prog.jpg', progressive=True)
    Image.fromarray(a).convert('CMYK').save(tmp_path / 'cmyk.jpg')
    good = write_jpeg(tmp_path / 'good.jpg', 4, 40, 48, 2, quality=90)
    raw = open(good, 'rb').read()
    (tmp_path / 'trunc.jpg').write_bytes(raw[:len(raw) // 2])
    out = np.zeros((40, 48, 3), np.uint8)

    def rc(name, h=40, w=48):
        return L.oadg_jpeg_decode_bgr(str(tmp_path / name).encode(), out.ctypes.data, h, w)
    assert rc('prog.jpg') == EUNSUPPORTED
    assert rc('cmyk.jpg') == EUNSUPPORTED
    assert L.oadg_jpeg_decode_bgr(_patched_411(tmp_path).encode(), np.zeros((32, 64, 3), np.uint8).ctypes.data,
                                  32, 64) == EUNSUPPORTED
    assert rc('trunc.jpg') == EFORMAT
    assert rc('missing.jpg') == EIO
    assert rc('good.jpg', 41, 48) == ESIZE
    assert rc('good.jpg') == OK and np.array_equal(out, pil_bgr(good))
    # the entropy stage reports the same codes and leaves a descriptor the device stage skips
    from oadg_amd import hip_ops
    cap = L.oadg_jpeg_coef_capacity(40, 48)
    assert cap == 3 * 48 * 48
    coef = np.zeros(cap, np.int16)
    desc = np.full(hip_ops.JPEG_DESC_BYTES, 0xAB, np.uint8)
    ncomp = desc[8:12].view(np.int32)
    for name, want in (('prog.jpg', EUNSUPPORTED), ('trunc.jpg', EFORMAT), ('good.jpg', OK)):
        got = L.oadg_jpeg_entropy_decode(str(tmp_path / name).encode(), 40, 48, coef.ctypes.data, cap, desc.ctypes.data)
        assert got == want and ncomp[0] == (3 if want == OK else 0), (name, got)
    assert L.oadg_jpeg_entropy_decode(good.encode(), 40, 48, coef.ctypes.data, 64, desc.ctypes.data) == ESIZE


@pytest.mark.gpu
def test_device_stage_is_byte_equal_to_pil(dev, tmp_path):
    """every file of the matrix through the entropy stage + one device batch per size, as CocoDataset.batch does it"""
    import torch
    from oadg_amd import hip_ops
    L = _lib()
    files = write_matrix(tmp_path)
    by_size = {}
    for path, h, w in files:
        by_size.setdefault((h, w), []).append(path)
    D = hip_ops.JPEG_DESC_BYTES
    for (h, w), paths in by_size.items():
        n, slot = len(paths), int(L.oadg_jpeg_coef_capacity(h, w))
        host = torch.zeros(n * D + 2 * n * slot, dtype=torch.uint8).pin_memory()
        base = host.numpy().ctypes.data
        for i, p in enumerate(paths):
            assert L.oadg_jpeg_entropy_decode(p.encode(), h, w, base + n * D + 2 * i * slot, slot, base + i * D) == OK, p
        d = host.to(dev)
        out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=dev)
        hip_ops.jpeg_pixels_bgr(d[n * D:].view(torch.int16), d[:n * D], out, slot)
        got = out.cpu().numpy()
        bad = [os.path.basename(p) for i, p in enumerate(paths) if not np.array_equal(got[i], pil_bgr(p))]
        assert not bad, ((h, w), bad)


def _voc_like_dataset(tmp_path, names, h, w, device):
    """a CocoDataset over the given files (one box each): CocoDataset.batch is the path under test"""
    import json
    from oadg_amd.datasets import CocoDataset
    images = [dict(id=i, file_name=n, height=h, width=w) for i, n in enumerate(names)]
    anns = [dict(id=i, image_id=i, category_id=1, iscrowd=0, area=100.0, bbox=[1.0, 1.0, 10.0, 10.0])
            for i in range(len(names))]
    with open(tmp_path / 'ann.json', 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name='car')]), f)
    return CocoDataset(ann_file=str(tmp_path / 'ann.json'), img_prefix=str(tmp_path), classes=('car',), device=device)


@pytest.mark.gpu
def test_mixed_batch_native_progressive_cmyk_png(dev, tmp_path):
    from PIL import Image
    a = noisy_image(7, 48, 64)
    write_jpeg(tmp_path / 'a.jpg', 1, 48, 64, 2, quality=90)
    Image.fromarray(a).save(tmp_path / 'p.jpg', progressive=True)
    Image.fromarray(a).convert('CMYK').save(tmp_path / 'c.jpg')
    write_jpeg(tmp_path / 'g.jpg', 2, 48, 64, 'L', quality=70)
    Image.fromarray(a).save(tmp_path / 'n.png')
    names = ['a.jpg', 'p.jpg', 'c.jpg', 'g.jpg', 'n.png']
    ds = _voc_like_dataset(tmp_path, names, 48, 64, dev)
    imgs, boxes, labels = ds.batch(range(len(names)))
    got = imgs.cpu().numpy()
    for i, n in enumerate(names):
        assert np.array_equal(got[i], pil_bgr(str(tmp_path / n))), n
    assert ds.jpeg_decodes == dict(native=2, pil=2)


@pytest.mark.gpu
def test_truncated_file_in_a_batch_raises_as_the_pil_path_does(dev, tmp_path, monkeypatch):
    from oadg_amd import datasets
    good = write_jpeg(tmp_path / 'a.jpg', 1, 48, 64, 2, quality=90)
    raw = open(good, 'rb').read()
    (tmp_path / 't.jpg').write_bytes(raw[:len(raw) // 2])
    ds = _voc_like_dataset(tmp_path, ['a.jpg', 't.jpg'], 48, 64, dev)
    errors = []
    for native in (False, True):
        monkeypatch.setattr(datasets, 'NATIVE_JPEG', native)
        with pytest.raises(Exception) as e:
            ds.batch([0, 1])
        errors.append(type(e.value))
    assert errors[0] is errors[1], errors
