"""GPU: Corrupt.batch of a resident batch for jpeg_compression and pixelate through csrc/recompress.hip
(oadg_recompress.py) equals corrupt() - Pillow - on the host image by image, byte for byte; no image of these inputs falls
back to the host, and numpy's global stream is not touched."""
import numpy as np
import pytest

from inputs import lowpass_image

NAMES = ('pixelate', 'jpeg_compression')

pytestmark = pytest.mark.gpu


def _compare(imgs, name, severity, seed=0):
    import torch
    from oadg_amd.pipelines.corrupt import Corrupt, corrupt
    ref = np.stack([corrupt(im, name, severity) for im in imgs])
    np.random.seed(seed)
    state = np.random.get_state()
    dev0, host0 = Corrupt.runs['device'], Corrupt.runs['host']
    out = Corrupt(name, severity).batch(torch.from_numpy(imgs).cuda()).cpu().numpy()
    after = np.random.get_state()
    bad = np.argwhere(out != ref)
    assert bad.size == 0, (name, severity, imgs.shape, len(bad), bad[:5].tolist(),
                           [(int(out[tuple(b)]), int(ref[tuple(b)])) for b in bad[:5]])
    # every image was finished on the device: zero fall-backs on these inputs
    assert (Corrupt.runs['device'], Corrupt.runs['host']) == (dev0 + len(imgs), host0)
    assert after[2:] == state[2:] and np.array_equal(after[1], state[1]), 'numpy stream differs after the batch'


def _pair(h, w, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, 256, (h, w, 3)).astype(np.uint8), np.full((h, w, 3), 128, np.uint8)])


@pytest.mark.parametrize('severity', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('name', NAMES)
def test_severity_sweep_random_and_grey(name, severity):
    _compare(_pair(61, 97, severity), name, severity)


@pytest.mark.parametrize('severity', [1, 3, 5])
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('h,w', [(9, 13), (33, 47), (5, 3), (40, 56)])
def test_small_odd_and_late_padded_sides(name, severity, h, w):
    """5 x 3: chroma 2 wide (replication), a 1 x 1 small image; 40 x 56: even and no multiple of 16 (the bottom edge of the
    chroma planes is padded after downsampling).  pixelate of 5 x 3 at severity 5 asks Pillow for a 1 x 0 image: the host
    path raises ValueError and so must the batch (the device declines it), nothing counted on the device"""
    import torch
    import oadg_recompress as R
    from oadg_amd.pipelines.corrupt import Corrupt, corrupt
    rs = np.random.RandomState(h * w + severity)
    imgs = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    if name == 'pixelate' and min(R.pixelate_size(h, w, severity)) < 1:
        assert (h, w, severity) == (5, 3, 5)
        before = dict(Corrupt.runs)
        with pytest.raises(ValueError):
            corrupt(imgs[0], name, severity)
        with pytest.raises(ValueError):
            Corrupt(name, severity).batch(torch.from_numpy(imgs).cuda())
        assert Corrupt.runs == before
        return
    _compare(imgs, name, severity)


@pytest.mark.parametrize('name', NAMES)
def test_batch_of_three_in_order(name):
    rs = np.random.RandomState(11)
    imgs = np.stack([lowpass_image(rs, 40, 56, 4), rs.randint(0, 256, (40, 56, 3)).astype(np.uint8),
                     np.full((40, 56, 3), 7, np.uint8)])
    _compare(imgs, name, 3, seed=123)


@pytest.fixture(scope='module')
def full_size():
    rs = np.random.RandomState(7)
    img = lowpass_image(rs, 1024, 2048, 6)
    img[::37] = rs.randint(0, 256, img[::37].shape)                 # some sharp rows as well
    img.setflags(write=False)
    return img


@pytest.mark.parametrize('severity', [3, 5])
@pytest.mark.parametrize('name', NAMES)
def test_full_size(full_size, name, severity):
    _compare(np.array(full_size[None]), name, severity, seed=1)          # (a writable copy: torch.from_numpy wants one)


def test_escape_hatch_gives_the_same_bytes_through_the_host_path(monkeypatch):
    import torch
    from oadg_amd.pipelines.corrupt import Corrupt
    x = torch.from_numpy(_pair(17, 23, 0)).cuda()
    for name in NAMES:
        d0, h0 = Corrupt.runs['device'], Corrupt.runs['host']
        a = Corrupt(name, 2).batch(x)
        assert (Corrupt.runs['device'], Corrupt.runs['host']) == (d0 + 2, h0)
        monkeypatch.setenv('OADG_DEVICE_CORRUPT', '0')
        b = Corrupt(name, 2).batch(x)
        monkeypatch.delenv('OADG_DEVICE_CORRUPT')
        assert (Corrupt.runs['device'], Corrupt.runs['host']) == (d0 + 2, h0 + 2)
        assert a.is_cuda and b.is_cuda and torch.equal(a, b)
        assert torch.equal(Corrupt(name, 0).batch(x), x)           # severity 0: the images, on the host path


def test_a_flagged_image_is_recomputed_on_the_host(monkeypatch):
    """the wrapper's flag read reports image 1 of 3: the result is still the host's bytes and that image counts as a host
    run.  The device's bytes of image 1 are replaced, so they are spoilt first to show that they are"""
    import torch
    import oadg_recompress as R
    from oadg_amd.pipelines.corrupt import Corrupt, corrupt
    rs = np.random.RandomState(2)
    imgs = rs.randint(0, 256, (3, 40, 56, 3)).astype(np.uint8)
    ref = np.stack([corrupt(im, 'jpeg_compression', 4) for im in imgs])
    real = R.jpeg_recompress

    def spoilt(x, quality):
        out, flags = real(x, quality)
        assert int(flags.sum()) == 0
        out[1] = 255 - out[1]
        return out, flags
    monkeypatch.setattr(R, 'jpeg_recompress', spoilt)
    monkeypatch.setattr(R, 'read_flags', lambda flags: np.array([0, 1, 0], np.int32))
    d0, h0 = Corrupt.runs['device'], Corrupt.runs['host']
    out = Corrupt('jpeg_compression', 4).batch(torch.from_numpy(imgs).cuda())
    assert (Corrupt.runs['device'], Corrupt.runs['host']) == (d0 + 2, h0 + 1)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), ref)


def test_a_declined_batch_raises_pillows_error():
    import torch
    from oadg_amd.pipelines.corrupt import Corrupt
    x = torch.full((1, 3, 3, 3), 9, dtype=torch.uint8).cuda()
    d0 = Corrupt.runs['device']
    with pytest.raises(ValueError):
        Corrupt('pixelate', 5).batch(x)
    assert Corrupt.runs['device'] == d0
    assert torch.equal(Corrupt('pixelate', 1).batch(x).cpu(), torch.full((1, 3, 3, 3), 9, dtype=torch.uint8))


def test_the_twins_agree_with_the_device_on_the_flags_and_the_planes_workspace():
    """the C ABI directly: a short workspace is refused, the flags come back zero, the bytes are the host twin's"""
    import torch
    import oadg_recompress as R
    from oadg_amd import _lib, staging
    rs = np.random.RandomState(5)
    imgs = rs.randint(0, 256, (2, 18, 6, 3)).astype(np.uint8)
    x = torch.from_numpy(imgs).cuda()
    out, flags = R.jpeg_recompress(x, 10)
    want, want_flags = R.jpeg_recompress_host(imgs, 10)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(flags.cpu().numpy(), want_flags)
    L = _lib.lib()
    need = int(L.oadg_jpeg_recompress_workspace_bytes(2, 18, 6))
    planes = torch.empty(need, dtype=torch.uint8, device='cuda')
    qt = staging.upload(R.quant_tables(10), x.device)
    rc = L.oadg_jpeg_recompress_u8(_lib.ptr(x), 2, 18, 6, _lib.ptr(qt), _lib.ptr(planes), need - 1, _lib.ptr(out),
                                   _lib.ptr(flags), _lib.stream_ptr())
    assert rc == -2                                                # OADG_ESIZE: nothing was launched
    oh, ow = R.pixelate_size(18, 6, 2)
    assert np.array_equal(R.pixelate(x, oh, ow).cpu().numpy(), R.pixelate_host(imgs, oh, ow))
