"""CPU: the device route of Corrupt.batch (csrc/corrupt.hip, pipelines/corrupt_device.py) - its C ABI, which names it
takes, and that CPU batches keep the host path.  The host-side tables the device path uploads (Gaussian weights, the
zoom grid, the motion blur's shifts) are checked here against scipy / the host loop; the bytes on the GPU are
tests/test_hip_corrupt.py's."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('oadg_corrupt_correlate1d', 'oadg_corrupt_epilogue', 'oadg_corrupt_defocus', 'oadg_corrupt_zoom_blur',
           'oadg_corrupt_snow_layer', 'oadg_corrupt_motion_blur_u8', 'oadg_corrupt_motion_blur_f64',
           'oadg_corrupt_snow_blend', 'oadg_corrupt_elastic', 'oadg_corrupt_hsv')


def test_header_and_ctypes_table_carry_the_corrupt_entry_points():
    src = open(os.path.join(ROOT, 'include', 'oadg_hip.h')).read()
    declared = set(re.findall(r'\b(oadg_corrupt_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    assert declared == set(ENTRIES)
    from oadg_amd import _lib
    assert set(ENTRIES) <= set(_lib.SIGNATURES)
    assert 'hipStream_t' in src or 'void* stream' in src
    for name in ENTRIES:
        assert _lib.SIGNATURES[name][1][-1] is _lib.vp, name            # the stream comes last


def test_device_and_host_names_partition_the_implemented_ones():
    from oadg_amd.pipelines import corrupt as C
    dev, host = set(C.DEVICE_CORRUPTIONS), set(C.HOST_CORRUPTIONS)
    assert not dev & host and dev | host == set(C.IMPLEMENTED)
    assert {'defocus_blur', 'zoom_blur', 'brightness', 'saturate', 'elastic_transform', 'motion_blur', 'snow',
            'gaussian_blur', 'glass_blur'} <= dev
    assert {'shot_noise', 'pixelate', 'jpeg_compression', 'spatter', 'frost'} <= host
    from oadg_amd.pipelines import corrupt_device as D
    assert tuple(D._DEVICE_FUNCS) == C.DEVICE_CORRUPTIONS


@pytest.mark.parametrize('name', ['zoom_blur', 'motion_blur', 'contrast'])
def test_a_cpu_batch_takes_the_host_path_and_is_counted(name):
    import torch
    from oadg_amd.pipelines.corrupt import Corrupt, corrupt
    rs = np.random.RandomState(3)
    imgs = rs.randint(0, 256, (2, 11, 17, 3)).astype(np.uint8)
    before = dict(Corrupt.runs)
    np.random.seed(5)
    out = Corrupt(name, 2).batch(torch.from_numpy(imgs))
    state = np.random.get_state()[1].copy()
    assert not out.is_cuda and out.dtype == torch.uint8
    assert Corrupt.runs['host'] == before['host'] + 2 and Corrupt.runs['device'] == before['device']
    np.random.seed(5)
    ref = np.stack([corrupt(im, name, 2) for im in imgs])
    assert np.array_equal(out.numpy(), ref) and np.array_equal(np.random.get_state()[1], state)


@pytest.mark.parametrize('sigma,truncate', [(1, 4.0), (6, 4.0), (np.float64(0.7), 4.0), (np.float64(1.5), 4.0),
                                            (np.float64(10.24), 3), (np.float64(20.48), 3), (np.float64(0.09), 3)])
def test_uploaded_gaussian_weights_are_scipys(sigma, truncate):
    from scipy.ndimage import gaussian_filter1d
    from oadg_amd.pipelines.corrupt_device import gaussian_weights
    w = gaussian_weights(sigma, truncate)
    r = len(w) // 2
    impulse = np.zeros(2 * r + 1)
    impulse[r] = 1.0
    # the impulse response of scipy's symmetric correlation is its weight vector, bit for bit
    assert np.array_equal(gaussian_filter1d(impulse, sigma, mode='constant', truncate=truncate), w)


@pytest.mark.parametrize('h,w', [(61, 97), (9, 13), (33, 47), (1024, 2048)])
def test_zoom_grid_matches_scipys_output_shape(h, w):
    from scipy.ndimage import zoom
    from oadg_amd.pipelines.corrupt_device import zoom_geometry
    for z in list(np.arange(1, 1.33, 0.03)) + [2, 2.5, 3, 4, 4.5]:
        (top, left, ch, cw), (Ho, Wo), _ = zoom_geometry(h, w, z)
        if h * w < 10000:
            assert zoom(np.zeros((ch, cw, 3), np.float32), (z, z, 1), order=1).shape == (Ho, Wo, 3)
        assert Ho >= h and Wo >= w and 0 <= top and 0 <= left


def test_motion_taps_reproduce_the_host_blur():
    from oadg_amd.pipelines import corrupt as C
    rs = np.random.RandomState(0)
    x = rs.randint(0, 256, (9, 13, 3)).astype(np.uint8)
    for angle in (-44.0, -3.5, 0.0, 27.0, -100.0):
        k = C._motion_kernel(15, 5)
        taps = C._motion_taps(x.shape, k.shape[0], angle)
        assert 0 < len(taps) <= k.shape[0]
        ref = np.zeros(x.shape)
        for i, (dx, dy) in enumerate(taps):
            yy = np.clip(np.arange(9) - dy, 0, 8)[:, None]
            xx = np.clip(np.arange(13) - dx, 0, 12)[None]
            ref = ref + k[i] * x[yy, xx]
        assert np.array_equal(C._motion_blur(x, 15, 5, angle), ref)
